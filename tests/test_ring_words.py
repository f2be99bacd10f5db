"""Ring words (hj_table.h RingWord, through hj_ring_word_layout_info: host-only arithmetic, no device): the 4-byte word a slot of a
wavefront's LDS ring holds on the slot-code road, word = (rel << 7) | code. For probeLength 1, 2, 3, 4, 8 and tables of 2^15,
2^27, 2^31, 2^32 slots EVERY displacement, EVERY high part a code holds and rel 0 and the largest the layout rule allows:
read back, stepped, compared. The code is held to hj_slot_codes_info's description of the byte the slot ends with."""
import itertools

import pytest

import htm_hashjoin_amd as hj

PROBES = (1, 2, 3, 4, 8)
TBITS = (15, 27, 31, 32)
EMPTY = 0xFFFFFFFF
REL_CAP = (1 << 25) - 1                      # a rel must be below it: the largest allowed is 2^25 - 2


def high_parts(tbits, info):
    """every high part a key of this table can have and a code can hold"""
    return range(min(info["hiCap"], 1 << (32 - tbits)))


def homes_of(tbits):
    """home slots whose walks stay inside the table, and the last ones, whose walks wrap at its end"""
    T = 1 << tbits
    return (0, 1, 12345, T // 2 + 77, T - 9, T - 3, T - 2, T - 1)


@pytest.mark.parametrize("probe,tbits", list(itertools.product(PROBES, TBITS)))
def test_every_word(probe, tbits):
    T = 1 << tbits
    info = hj.slot_codes_info(T, probe)
    dbits = info["dbits"]
    assert info["hiCap"] == 128 >> dbits
    words = {}
    for rel in (0, REL_CAP - 1):
        for hi in high_parts(tbits, info):
            for home in homes_of(tbits):
                key = (hi << tbits) | home if tbits < 32 else home
                at_home = hj.ring_word_info(T, probe, rel, key)["word"]
                for d in range(probe):
                    w = hj.ring_word_info(T, probe, rel, key, d)
                    tag = (probe, tbits, rel, hi, home, d)
                    # decode(encode) is the identity, at the slot the tuple stands at (wrapped at the table's end)
                    assert w["slot"] == (home + d) % T and w["key"] == key, (tag, w)
                    assert (w["rel"], w["relCap"], w["empty"]) == (rel, REL_CAP, EMPTY), (tag, w)
                    # the code is the byte the slot ends with: (hi << dbits) | d, 7 bits
                    assert w["code"] == (hi << dbits) | d and w["code"] < 0x80, (tag, w)
                    # a step keeps the key (above), adds one to d and nothing else: no carry into the high part or rel
                    assert w["word"] == at_home + d == (rel << 7) | (hi << dbits) | d, (tag, w)
                    assert w["triesLeft"] == probe - d >= 1, (tag, w)
                    # no reachable word is the empty pattern, and every one orders below it
                    assert w["word"] < EMPTY, (tag, w)
                    words[(rel, key, d)] = w["word"]
                # the budget is decided BEFORE the step: the word one step past the last try does not exist
                with pytest.raises(hj.HashJoinError):
                    hj.ring_word_info(T, probe, rel, key, probe)
    # order follows rel, whatever the codes: every word of rel 0 is below every word of the largest rel
    assert max(w for (rel, _, _), w in words.items() if rel == 0) < min(w for (rel, _, _), w in words.items() if rel)


@pytest.mark.parametrize("probe", PROBES)
def test_order_is_that_of_rel(probe):
    """neighbouring rels under the largest and the smallest code: (rel, any code) < (rel + 1, any code)"""
    T = 1 << 15
    info = hj.slot_codes_info(T, probe)
    lo_key, hi_key = 5, ((info["hiCap"] - 1) << 15) | 5
    for rel in (0, 1, 63, 64, 511, 512, 1 << 17, REL_CAP - 2):
        top = hj.ring_word_info(T, probe, rel, hi_key, probe - 1)["word"]        # the largest code there is
        nxt = hj.ring_word_info(T, probe, rel + 1, lo_key, 0)["word"]            # code 0
        assert top < nxt, (probe, rel)
        assert hj.ring_word_info(T, probe, rel, lo_key, 0)["word"] >> 7 == rel


def test_the_layout_rule_refuses_what_a_word_cannot_hold():
    """rel = 2^25 - 1 with code 127 would BE the empty pattern; the rule stops one short of it, whatever the code"""
    T = 1 << 15
    assert hj.ring_word_info(T, 4, REL_CAP - 1, 31 << 15 | 9, 3)["word"] == EMPTY - 128
    for rel in (REL_CAP, REL_CAP + 1, 1 << 31, 0xFFFFFFFF):
        with pytest.raises(hj.HashJoinError) as e:
            hj.ring_word_info(T, 4, rel, 9)
        assert e.value.status == hj.HJ_ERR_INVALID and e.value.partial["relCap"] == REL_CAP


def test_what_the_road_never_makes():
    for bad in ((0, 4, 0, 9, 0), (3 << 20, 4, 0, 9, 0), (1 << 33, 4, 0, 9, 0), (1 << 20, 0, 0, 9, 0),
                (1 << 15, 129, 0, 9, 0),                 # no code at this probeLength
                (1 << 15, 4, 0, 32 << 15 | 9, 0),        # hi = hiCap: a key without a code (cause 4 of the forced road)
                (1 << 15, 4, 0, 0xFFFFFFFF, 0)):
        with pytest.raises(hj.HashJoinError):
            hj.ring_word_info(*bad)
    assert hj.lib.hj_ring_word_layout_info(1 << 15, 4, 0, 9, 0, None) == hj.HJ_ERR_INVALID
