"""The generator of the relational fuzz (fuzz_tables.py) and the harness around it, without a device: over the seeds the
GPU tests use by default the problems must hold what the tests are about -- counted and asserted here, as
test_the_input_cannot_pass_vacuously does for its fixed data -- and stay under the cap on the inner pairs; the host twins
of the device calls (pairs_where_host, pairs_asof_host, key_groups_host, key_hash2_host) are held to the models on the
candidate lists and key columns of the same problems; and the slot-code cases of test_gpu_fuzz.py are shown able to stay
on their road."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj

import asof_common as asc
import fuzz_relations as fr
import fuzz_tables as ft
import groups_common as gc
import keys2_common as k2
import where_common as wc


@pytest.fixture(scope="module")
def world():
    """every problem of the default seeds, with the model's parts: (block, case, problem, parts of the plain inner join)"""
    out = []
    for block in range(ft.BLOCKS):
        for case, p in ft.problems(block):
            out.append((block, case, p, wc.model_join("inner", p.r_rowkeys, p.s_rowkeys, [])[1]))
    return out


def winners(p, where):
    """{s: r} of the as-of join, and the model's parts"""
    rows, parts = asc.model_join_asof("inner", p.r_rowkeys, p.s_rowkeys, where, p.asof_model)
    return dict(rows), parts


def test_the_generator_cannot_pass_vacuously(world):
    seen = dict.fromkeys(("pairs", "no_pairs", "several_eligible", "tied_winners", "empty_slice", "all_null_keyed", "no_groups",
                          "where_moves_winner", "empty_side", "where", "asof", "plain_keys", "sliced"), 0)
    kinds, hows, ops, asof_ops = {}, {}, {}, {}
    most = 0
    for block, case, p, parts in world:
        inner = parts["inner"]
        assert len(inner) == p.inner_pairs <= ft.PAIR_CAP, (block, case, len(inner))
        most = max(most, len(inner))
        seen["pairs" if inner else "no_pairs"] += 1
        seen["empty_side"] += p.n_r == 0 or p.n_s == 0
        seen["where"] += bool(p.where)
        seen["asof"] += p.asof is not None
        seen["plain_keys"] += p.plain_keys and p.n_r > 0 and p.n_s > 0
        seen["sliced"] += p.n_s > p.step
        for w in p.widths:
            kinds[w] = kinds.get(w, 0) + 1
        hows[p.how] = hows.get(p.how, 0) + 1
        for term in p.where_model:
            ops[term[1]] = ops.get(term[1], 0) + 1
        if inner and p.n_s > p.step:
            hit = {s // p.step for s, _ in inner}
            seen["empty_slice"] += len(hit) < -(-p.n_s // p.step)
        for keys, n in ((p.r_rowkeys, p.n_r), (p.s_rowkeys, p.n_s)):
            seen["all_null_keyed"] += n > 0 and all(k is None for k in keys)
        seen["no_groups"] += p.nulls == "drop" and p.n_s > 0 and gc.model_groups(gc.model_keys(p.s_model, "drop"))["n_groups"] == 0
        if p.asof_model is not None:
            asof_ops[p.asof_model[1]] = asof_ops.get(p.asof_model[1], 0) + 1
            best, model = winners(p, p.where_model)
            eligible = {}
            for (s, r), ok in zip(model["cand"], model["eligible"]):
                if ok:
                    eligible.setdefault(s, []).append(r)
            r_values = p.asof_model[2]
            seen["several_eligible"] += any(len(rs) > 1 for rs in eligible.values())
            seen["tied_winners"] += any(sum(bool(r_values[r] == r_values[best[s]]) for r in rs) > 1 for s, rs in eligible.items())
            if p.where_model:
                plain, _ = winners(p, [])
                seen["where_moves_winner"] += any(s in plain and plain[s] != r for s, r in best.items())
    print("problems", len(world), "most inner pairs", most, seen)
    print("key kinds", kinds, "hows", hows, "where ops", ops, "asof ops", asof_ops)
    assert most > 10000, "no problem near the sizes where the pairs outgrow a slice's planes"
    for what, count in seen.items():
        assert count >= 3, (what, count)
    assert set(kinds) == set(ft.KEY_KINDS) and min(kinds.values()) >= 3, kinds
    assert set(hows) == set(wc.HOWS) and min(hows.values()) >= 3, hows
    assert set(ops) == set(wc.OPS) and min(ops.values()) >= 3, ops
    assert set(asof_ops) == set(asc.ASOF_OPS) and min(asof_ops.values()) >= 3, asof_ops


def candidate_maps(parts, lo=0, n=None):
    """the candidate pairs whose S row lies in [lo, lo + n), as the two maps a device call gets, S rows counted from 0"""
    cand = [(s, r) for s, r in parts["cand"] if n is None or lo <= s < lo + n]
    return (np.array([s for s, _ in cand], dtype=np.uint32), np.array([r for _, r in cand], dtype=np.uint32))


def slice_of(value, lo, n):
    """rows [lo, lo + n) of one side of a term as the wrappers take it"""
    if isinstance(value, hj.KeyColumn):
        return hj.KeyColumn(value.values[lo:lo + n], None if value.valid is None else value.valid[lo:lo + n])
    return value[lo:lo + n]


def slice_term(term, lo, n):
    s, op, r, s_valid, r_valid = term
    return (s[lo:lo + n], op, r, None if s_valid is None else s_valid[lo:lo + n], r_valid)


def same_call(got, want, map_s, map_r, tag):
    assert got["info"] == want["info"], (tag, got["info"], want["info"])
    keep = want["keep"]
    assert np.array_equal(got["s_idx"], map_s[keep]) and np.array_equal(got["r_idx"], map_r[keep]), (tag, "the kept pairs, in input order")
    assert np.array_equal(got["s_marks"], want["s_marks"]) and np.array_equal(got["r_marks"], want["r_marks"]), (tag, "marks")


def slices_of(p):
    """the whole S side, and the drawn slice that ends it (it starts in the middle of validity words and is the short one)"""
    out = [(0, p.n_s)]
    if 0 < p.step < p.n_s:
        lo = (p.n_s - 1) // p.step * p.step
        out.append((lo, p.n_s - lo))
    return out


def test_pairs_where_host_against_the_model(world):
    done = 0
    for block, case, p, parts in world:
        if not p.where or p.n_r == 0 or p.n_s == 0:
            continue
        for lo, n in slices_of(p):
            map_s, map_r = candidate_maps(parts, lo, n)
            terms = [(slice_of(s, lo, n), op, r) for s, op, r in p.where]
            want = wc.model_call(map_s, map_r, lo, n, p.n_r, [slice_term(t, lo, n) for t in p.where_model])
            got = hj.pairs_where_host(map_s, map_r, lo, terms, marks=True)
            same_call(got, want, map_s, map_r, ft.tag_of(p, block, case, lo=lo, n=n))
            done += 1
    assert done >= 20, done


def test_pairs_asof_host_against_the_model(world):
    done = 0
    for block, case, p, parts in world:
        if p.asof is None or p.n_r == 0 or p.n_s == 0:
            continue
        for lo, n in slices_of(p):
            map_s, map_r = candidate_maps(parts, lo, n)
            s, op, r = p.asof
            want = asc.model_call(map_s, map_r, lo, n, p.n_r, slice_term(p.asof_model, lo, n))
            got = hj.pairs_asof_host(map_s, map_r, lo, (slice_of(s, lo, n), op, r), marks=True)
            tag = ft.tag_of(p, block, case, lo=lo, n=n)
            same_call(got, want, map_s, map_r, tag)
            assert np.array_equal(got["best_row"], want["best_row"]), (tag, "best_row")
            done += 1
    assert done >= 20, done


def test_key_groups_host_against_the_model(world):
    for block, case, p, _ in world:
        for nulls in ft.NULLS:
            for key_mask in dict.fromkeys((0, p.key_mask)):
                want = gc.model_groups(gc.model_keys(p.s_model, nulls))
                gc.same(hj.key_groups_host(p.s_keys, nulls=nulls, key_mask=key_mask), want, ft.tag_of(p, block, case, nulls_run=nulls, mask_run=key_mask))


def test_key_hash2_host_against_the_model(world):
    for block, case, p, _ in world:
        for model, lead in ((p.r_model, 0), (p.s_model, 3)):
            if not model[0].items:
                continue
            for nulls_equal in (False, True):
                cols = [c._replace(nulls_equal=nulls_equal) for c in model]
                got = hj.key_hash2_host([k2.key_column(c, lead=lead) for c in cols], key_mask=p.key_mask)
                assert np.array_equal(got, k2.model_words(cols, p.key_mask)), ft.tag_of(p, block, case, nulls_equal_run=nulls_equal, lead=lead)


def test_the_slot_code_cases_can_stay_on_their_road():
    """test_slot_code_road_on_random_near_sorted_relations asks that half of its cases without an uncodable key stay on the
    road. What can push a case off it is the dirty log's overflow, which needs disorder beyond what the rings hold: the
    `shuffle` relation of test_log_overflow_stays_a_cause has none, and W up to 100 is what the locality sample calls
    tight. So per test id, the cases drawn with W < 300 must be more than half of those without an uncodable key."""
    for block in range(4):
        rng = np.random.default_rng(20265000 + block)
        tight = codable = 0
        for case in range(block, 36, 4):
            n, plen, idx_base, R, S, w, hi = fr.slot_code_case(rng)
            assert R.size == n and int(R.max()) < 0xFFFFFFFF and int(R.min()) > 0
            assert bool((R >= np.uint64(hi["keyLimit"])).any()) == (hi["over"] > 0)
            if not hi["over"]:
                codable += 1
                tight += w < 300
        print("block", block, "codable", codable, "with W < 300", tight)
        assert codable >= 5 and 4 * tight >= 3 * codable, (block, tight, codable)
