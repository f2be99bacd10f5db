"""key_hash2 and pairs_verify2 on an MI355X. The hash on the device equals key_hash2_host over the matrix the host hash is
checked on against the header's wording (test_keys2_abi.py), both sides read from their own pointers. pairs_verify2 runs on
hand-made candidate lists whose every entry is decided by the model in keys2_common: the kept multiset, both mark planes and
verify_info. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj

from gpu_harness import dev, plane_bits, row_bits  # noqa: F401
from keys2_common import MASKS, ROWS, ModelCol, hash_matrix, key_column
from keys_common import key_words, murmur3_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
NE = hj.HJ_KEY_NULLS_EQUAL


def descriptor(s, r, width, flags):
    """the tuple key_hash2 / pairs_verify2 take, from the (values, offsets, validity) of each side (None: not in use)"""
    s, r = s or (0, 0, 0), r or (0, 0, 0)
    return (s[0], r[0], width, s[1], r[1], s[2], r[2], flags)


@pytest.mark.parametrize("n", ROWS)
def test_device_hash_equals_host_hash(dev, n):
    """every column list of the host test's matrix; S from the S pointers, R (other data) from the R pointers"""
    rng = np.random.default_rng(77 + n)
    models_s, models_r = hash_matrix(rng, n), hash_matrix(rng, n)
    d_out = dev.alloc(8 * n)
    for model_s, model_r in zip(models_s, models_r):
        cols_s = [key_column(c, lead=k % 4) for k, c in enumerate(model_s)]
        cols_r = [key_column(c, lead=(k + 1) % 4) for k, c in enumerate(model_r)]
        desc = [descriptor(dev.column(s), dev.column(r), s.width, NE if s.nulls_equal else 0) for s, r in zip(cols_s, cols_r)]
        for key_mask in MASKS:
            for side, cols in ((hj.HJ_KEY_SIDE_S, cols_s), (hj.HJ_KEY_SIDE_R, cols_r)):
                dev.ctx.copy_h2d(d_out, np.full(n, 0xDEAD, dtype=U64))
                dev.ctx.key_hash2(desc, side, n, d_out, key_mask)
                dev.ctx.synchronize()
                assert np.array_equal(dev.get(d_out, n, U64), hj.key_hash2_host(cols, key_mask=key_mask)), (
                    [(c.width, c.nulls_equal) for c in model_s], n, key_mask, side)
    dev.release()


def test_device_hash_of_plain_columns_equals_key_hash(dev):
    """the compatibility property on the device: no offsets, no validity, flags 0 -> what hj_key_hash_dev writes. Both
    entry points run one kernel, so the property rests on the header's wording, restated in keys_common.py"""
    n = 5000
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, 1 << 63, n, dtype=np.uint64), rng.integers(0, 1 << 16, n).astype(np.uint16)
    d_a, d_b, d_old, d_new = dev.put(a), dev.put(b), dev.alloc(8 * n), dev.alloc(8 * n)
    dev.ctx.key_hash([(d_a, 0, 8), (d_b, 0, 2)], hj.HJ_KEY_SIDE_S, n, d_old, 0xFFF)
    dev.ctx.key_hash2([(d_a, 0, 8), (d_b, 0, 2)], hj.HJ_KEY_SIDE_S, n, d_new, 0xFFF)
    dev.ctx.synchronize()
    assert np.array_equal(dev.get(d_new, n, U64), dev.get(d_old, n, U64))
    assert np.array_equal(dev.get(d_new, n, U64), hj.key_hash_host([a, b], key_mask=0xFFF))
    assert np.array_equal(dev.get(d_new, n, U64), murmur3_words(key_words([a, b]), 0xFFF))
    dev.release()


# ---- pairs_verify2 -----------------------------------------------------------------------------------------------------------
LONG = bytes(range(256)) + b"!"                                                # 257 bytes
SPECIAL = [None, b"", b"ab", b"abc", b"x" * 30 + b"1", b"x" * 30 + b"2",       # prefix; equal lengths, the last byte differs
           b"wxyzA123", b"wxyzB123",                                           # ... the first byte past a word boundary differs
           LONG, LONG[:-1] + b"?", b"q", None, b"ab", b""]


def equal(cols_s, cols_r, flags, i, j):
    """the header's column equality on the model's rows"""
    for s, r, f in zip(cols_s, cols_r, flags):
        a, b = s.items[i], r.items[j]
        if a is None or b is None:
            if not (a is None and b is None and f):
                return False
        elif a != b:
            return False
    return True


def verify_case(composite, flags):
    """S rows, R rows and about 3000 candidates: every pair of the special rows, random pairs, HJ_NO_ROW and out-of-range
    entries. Returns the model columns, the raw maps and, per candidate, 'kept' / 'rejected' / 'dropped'."""
    rng = np.random.default_rng(41 + composite + 2 * sum(flags))
    pool = [rng.integers(97, 100, size=int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 10, 12)]
    s_str = SPECIAL + [pool[k] for k in rng.integers(0, 12, 150)]
    r_str = SPECIAL[::-1] + [pool[k] for k in rng.integers(0, 12, 120)]
    n_s, n_r = len(s_str), len(r_str)
    cols_s, cols_r = [ModelCol(0, s_str, False)], [ModelCol(0, r_str, False)]
    if composite:       # a nullable 8-byte column in front: few values, a fifth NULL, so every combination occurs
        ints = [int(v).to_bytes(8, "little") for v in (0, 1 << 40)]
        pick = lambda n: [None if rng.random() < 0.2 else ints[rng.integers(0, 2)] for _ in range(n)]       # noqa: E731
        cols_s, cols_r = [ModelCol(8, pick(n_s), False)] + cols_s, [ModelCol(8, pick(n_r), False)] + cols_r
    base = 1000
    k = len(SPECIAL)
    pairs = [(i, j) for i in range(k) for j in range(k)]
    pairs += list(zip(rng.integers(0, n_s, 2700).tolist(), rng.integers(0, n_r, 2700).tolist()))
    map_s = np.array([i + base for i, _ in pairs], dtype=np.uint32)
    map_r = np.array([j for _, j in pairs], dtype=np.uint32)
    bad = rng.permutation(len(pairs))[:120]
    map_s[bad[:20]] = hj.NO_ROW
    map_r[bad[20:40]] = hj.NO_ROW
    map_s[bad[40:60]] = base + n_s + rng.integers(0, 5, 20)                     # at or behind sRows
    map_s[bad[60:80]] = rng.integers(0, base, 20)                               # in front of the base
    map_r[bad[80:100]] = n_r + rng.integers(0, 1 << 20, 20)
    map_s[bad[100:120]] = hj.NO_ROW
    map_r[bad[100:120]] = hj.NO_ROW
    fate = []
    for es, er in zip(map_s.tolist(), map_r.tolist()):
        if es == hj.NO_ROW or er == hj.NO_ROW or not base <= es < base + n_s or er >= n_r:
            fate.append("dropped")
        else:
            fate.append("kept" if equal(cols_s, cols_r, flags, es - base, er) else "rejected")
    return cols_s, cols_r, base, map_s, map_r, np.array(fate)


def case_by_the_model(composite, flags):
    """verify_case and what its list must contain, decided by the model alone (needs no device)"""
    cols_s, cols_r, base, map_s, map_r, fate = verify_case(composite, flags)
    n_s, n_r, n = len(cols_s[0].items), len(cols_r[0].items), map_s.size
    assert 2048 < n <= 3072, "two full workgroups and a partial one"
    kept = fate == "kept"
    want = np.sort((map_s[kept].astype(U64) << U64(32)) | map_r[kept].astype(U64))
    want_s, want_r = row_bits(map_s[kept] - base, n_s), row_bits(map_r[kept], n_r)
    print("candidates", n, "kept", int(kept.sum()), "rejected", int((fate == "rejected").sum()), "dropped", int((fate == "dropped").sum()))
    assert kept.sum() >= 40 and (fate == "rejected").sum() > 100 and (fate == "dropped").sum() >= 100
    # what the list must contain, by the model
    s_str, r_str = cols_s[-1].items, cols_r[-1].items
    seen = {(s_str[i - base], r_str[j], f) for i, j, f in zip(map_s.tolist(), map_r.tolist(), fate.tolist()) if f != "dropped"}
    null_fate = "kept" if flags[-1] and not composite else None
    for a, b in ((None, b""), (b"", None), (b"ab", None), (None, b"ab")):
        assert (a, b, "rejected") in seen, (a, b)                               # "" against NULL; NULL on one side only
    if null_fate:
        assert (None, None, "kept") in seen
    if not any(flags):
        assert (None, None, "rejected") in seen and (None, None, "kept") not in seen
    assert (b"ab", b"abc", "rejected") in seen and (b"abc", b"ab", "rejected") in seen
    assert (SPECIAL[4], SPECIAL[5], "rejected") in seen and (SPECIAL[6], SPECIAL[7], "rejected") in seen
    assert (LONG, SPECIAL[9], "rejected") in seen
    if not composite:
        assert (b"", b"", "kept") in seen and (LONG, LONG, "kept") in seen and (SPECIAL[4], SPECIAL[4], "kept") in seen

    return cols_s, cols_r, base, map_s, map_r, fate, kept, want, want_s, want_r


@pytest.mark.parametrize("composite,flags", [(False, (0,)), (False, (NE,)), (True, (0, 0)), (True, (NE, NE)), (True, (NE, 0)), (True, (0, NE))])
def test_pairs_verify2_against_the_model(dev, composite, flags):
    cols_s, cols_r, base, map_s, map_r, fate, kept, want, want_s, want_r = case_by_the_model(composite, flags)
    n_s, n_r, n = len(cols_s[0].items), len(cols_r[0].items), map_s.size
    s_str = cols_s[-1].items
    ks, kr =[key_column(c, lead=1) for c in cols_s], [key_column(c, lead=2) for c in cols_r]
    if not composite:       # the same string at different alignments on the two sides, among the kept pairs
        so, ro = ks[0].offsets, kr[0].offsets
        assert any((int(so[i - base]) - int(ro[j])) % 4 and s_str[i - base] for i, j in zip(map_s[kept].tolist(), map_r[kept].tolist()))
    desc = [descriptor(dev.column(s), dev.column(r), s.width, f) for s, r, f in zip(ks, kr, flags)]
    d_ms, d_mr = dev.put(map_s), dev.put(map_r)
    words_s, words_r = (n_s + 31) // 32, (n_r + 31) // 32

    def run(capacity, outputs=True):
        d_sm, d_rm = dev.put(np.zeros(words_s, dtype=np.uint32)), dev.put(np.zeros(words_r, dtype=np.uint32))
        d_ks, d_kr = (dev.put(np.full(capacity + 8, 0xABABABAB, dtype=np.uint32)) for _ in range(2)) if outputs else (0, 0)
        dev.ctx.pairs_verify2(d_ms, d_mr, n, base, n_s, n_r, desc, d_ks, d_kr, capacity, d_sm, d_rm)
        info = dev.ctx.verify_info()
        got_s, got_r = (dev.get(d, capacity + 8) for d in (d_ks, d_kr)) if outputs else (None, None)
        return info, got_s, got_r, plane_bits(dev.get(d_sm, words_s), n_s), plane_bits(dev.get(d_rm, words_r), n_r)

    # room for everything
    info, got_s, got_r, marks_s, marks_r = run(n)
    assert (info[0], info[1], info[3]) == (want.size, want.size, int((fate == "dropped").sum()))
    assert np.array_equal(np.sort((got_s[:want.size].astype(U64) << U64(32)) | got_r[:want.size].astype(U64)), want)
    assert (got_s[want.size:] == 0xABABABAB).all() and (got_r[want.size:] == 0xABABABAB).all(), "nothing behind the kept pairs"
    assert np.array_equal(marks_s, want_s) and np.array_equal(marks_r, want_r)
    # a capacity below the kept count: the count and the marks are complete, the written pairs are kept ones
    cap = want.size // 3
    info, got_s, got_r, marks_s, marks_r = run(cap)
    assert (info[0], info[1], info[3]) == (want.size, cap, int((fate == "dropped").sum()))
    some = (got_s[:cap].astype(U64) << U64(32)) | got_r[:cap].astype(U64)
    uniq, counts = np.unique(want, return_counts=True)
    got_u, got_c = np.unique(some, return_counts=True)
    pos = np.searchsorted(uniq, got_u)
    assert (pos < uniq.size).all() and np.array_equal(uniq[pos], got_u) and (got_c <= counts[pos]).all()
    assert (got_s[cap:] == 0xABABABAB).all() and (got_r[cap:] == 0xABABABAB).all(), "nothing at or behind the capacity"
    assert np.array_equal(marks_s, want_s) and np.array_equal(marks_r, want_r)
    # a mark-only pass
    info, _, _, marks_s, marks_r = run(0, outputs=False)
    assert (info[0], info[1], info[3]) == (want.size, 0, int((fate == "dropped").sum()))
    assert np.array_equal(marks_s, want_s) and np.array_equal(marks_r, want_r)
    dev.release()


def test_verify_info_reports_the_last_call_of_either_entry(dev):
    """pairs_verify, then pairs_verify2 on the same plain column: the same kept pairs, and the record is the last call's"""
    rng = np.random.default_rng(12)
    s, r = rng.integers(0, 50, 700).astype(np.uint64), rng.integers(0, 50, 600).astype(np.uint64)
    map_s, map_r = rng.integers(0, 700, 2500).astype(np.uint32), rng.integers(0, 600, 2500).astype(np.uint32)
    keep = s[map_s] == r[map_r]
    d_s, d_r, d_ms, d_mr = dev.put(s), dev.put(r), dev.put(map_s), dev.put(map_r)
    d_ks, d_kr = dev.alloc(4 * 2500), dev.alloc(4 * 2500)
    dev.ctx.pairs_verify(d_ms, d_mr, 2500, 0, 700, 600, [(d_s, d_r, 8)], d_ks, d_kr, 2500)
    old = dev.ctx.verify_info()
    old_pairs = np.sort((dev.get(d_ks, old[0]).astype(U64) << U64(32)) | dev.get(d_kr, old[0]).astype(U64))
    dev.ctx.pairs_verify2(d_ms, d_mr, 1500, 0, 700, 600, [(d_s, d_r, 8)], d_ks, d_kr, 2500)
    assert dev.ctx.verify_info()[0] == int(keep[:1500].sum()) != old[0]
    dev.ctx.pairs_verify2(d_ms, d_mr, 2500, 0, 700, 600, [(d_s, d_r, 8)], d_ks, d_kr, 2500)
    new = dev.ctx.verify_info()
    assert (new[0], new[1], new[3]) == (old[0], old[1], old[3]) == (int(keep.sum()), int(keep.sum()), 0)
    assert np.array_equal(np.sort((dev.get(d_ks, new[0]).astype(U64) << U64(32)) | dev.get(d_kr, new[0]).astype(U64)), old_pairs)
    dev.release()
