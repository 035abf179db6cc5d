"""The 2048 agents' one greedy rule (pulselib_amd/agents/tfe_common.py: greedy_scan_on_host and its vectorised twin) as the three
agent-level statements take it: greedy_on_host (a table entry), greedy_after_on_host (a table of afterstate values) and
greedy_nt_on_host (an n-tuple network), on one set of stated q and stated coin words."""
import numpy as np

TIE_SEED = 7
# board A: a 2 in cell 0 and a 4 in cell 5.  Every move changes it, no move merges (the four rewards are 0), and the four afterstates
# differ.  Bit 31 of words 0..2 of Philox(TIE_SEED, key of A, round): the coins of actions 1, 2, 3.
KEY_A = 0x200001
COINS_A = {0: (1, 1, 1), 1: (0, 0, 0), 3: (0, 0, 1), 4: (1, 0, 1), 5: (1, 1, 0), 6: (0, 1, 0), 7: (1, 0, 0), 15: (0, 1, 1)}
WORDS_A = {1: [0x3F6C3E5E, 0x507A689A, 0x168FD762, 0x4F3921B0], 7: [0x9C67ED50, 0x48199C1D, 0x3E78FA88, 0x49D55DDF]}
# board B: a 2 in cell 0 and a 4 in cell 8: the move to the left changes nothing, the other three do, again without a merge
KEY_B = 0x200000001
COINS_B = {0: (0, 1, 0), 4: (1, 0, 0), 12: (0, 0, 0), 14: (0, 0, 1)}
TUPLES = ((0, 3, 4, 8, 11, 12),)                # one table, no symmetry: the afterstates of A and of B read distinct weights

# (q of the four moves, round, the action by hand)
CASES_A = [
    ((1, 3, 2, 0), 0, 1),                       # no tie: the largest q, whatever the coins
    ((2, 2, 1, 0), 7, 1),                       # q1 = q0 and the coin of action 1 is set
    ((2, 2, 1, 0), 1, 0),                       # ... and clear
    ((5, 5, 5, 1), 6, 2),                       # three equal: coins 0 1 0 -- action 1 stays out, action 2 replaces action 0
    ((5, 5, 5, 1), 7, 1),                       # coins 1 0 0
    ((5, 5, 5, 1), 5, 2),                       # coins 1 1 0: action 1 takes it, then action 2
    ((5, 5, 5, 1), 4, 1),                       # coins 1 0 1: the coin of action 3 plays no part, its q is smaller
    ((5, 5, 5, 1), 3, 0),                       # coins 0 0 1
    ((1, 1, 2, 0), 7, 2),                       # a tie's coin does not matter to the larger q after it
    ((0, 0, 0, 0), 3, 3),                       # four equal, coins 0 0 1
    ((0, 0, 0, 0), 15, 3),                      # coins 0 1 1
]
# ... for the n-tuple rule, where only the moves that change the board are candidates: on B the candidates are 1, 2, 3
CASES_B = [
    ((9, 1, 1, 0), 12, 1),                      # action 0 has the largest q and is no candidate; coins 0 0 0: the first candidate stays
    ((9, 1, 1, 0), 4, 1),                       # coins 1 0 0: the first candidate needs no coin
    ((9, 1, 1, 0), 0, 2),                       # coins 0 1 0
    ((9, 1, 3, 3), 14, 3),                      # coins 0 0 1
    ((9, 1, 3, 3), 12, 2),
]


def _board(key):
    return np.array([(1 << ((key >> (4 * i)) & 15)) & ~1 for i in range(16)]).reshape(4, 4)


def _nt_action(key, q, round):
    """greedy_nt_on_host on one board whose four afterstates have the values q (no merge: q = gamma * V = V)"""
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    after, scores = nt.moves_on_host([key])
    idx = nt.feature_indices_on_host(after.reshape(-1), TUPLES, False).reshape(-1)
    assert not scores.any() and len(set(idx.tolist())) == len(set(after.reshape(-1).tolist()))
    w = np.zeros(nt.tuple_offsets(TUPLES)[1], dtype=np.float32)
    w[idx] = q
    out = nt.greedy_nt_on_host([key], w, TUPLES, False, 1.0, TIE_SEED, round)
    assert out["q"][0].tolist() == [float(x) for x in q]
    return int(out["action"][0])


def test_the_three_greedy_rules_agree_on_stated_values():
    from pulselib_amd.agents import tfe_common as common
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    assert mc.pack_board(_board(KEY_A)) == KEY_A and mc.pack_board(_board(KEY_B)) == KEY_B
    for key, coins in ((KEY_A, COINS_A), (KEY_B, COINS_B)):                 # the coins are the stated ones, in both forms of Philox
        for r, bits in coins.items():
            assert tuple(w >> 31 for w in mc.philox4x32(TIE_SEED, key, r)[:3]) == bits, (hex(key), r)
            assert nt.philox_many_on_host(TIE_SEED, [key], r)[0].tolist() == mc.philox4x32(TIE_SEED, key, r)
    assert all(mc.philox4x32(TIE_SEED, KEY_A, r) == words for r, words in WORDS_A.items())
    after, rewards = mc.afterstates_on_host(_board(KEY_A))
    assert len(set(after)) == 4 and rewards == [0, 0, 0, 0]
    for q, r, want in CASES_A:
        entry = ([1] * 4, list(q))                                          # q(s, a) = sum / cnt
        table = {k: ([1, 0, 0, 0], [x, 0, 0, 0]) for k, x in zip(after, q)}  # v(afterstate) = sum[0] / cnt[0]
        got = (mc.greedy_on_host(entry, KEY_A, TIE_SEED, r), mc.greedy_after_on_host(_board(KEY_A), table, 1.0, 0, TIE_SEED, r)[0],
               _nt_action(KEY_A, q, r), common.greedy_scan_on_host(q, lambda: mc.philox4x32(TIE_SEED, KEY_A, r)))
        assert got == (want,) * 4, (q, r, got)
    cand = (nt.moves_on_host([KEY_B])[0][0] != np.uint64(KEY_B)).tolist()
    assert cand == [False, True, True, True]
    for q, r, want in CASES_B:
        got = (_nt_action(KEY_B, q, r), common.greedy_scan_on_host(q, lambda: mc.philox4x32(TIE_SEED, KEY_B, r), cand))
        assert got == (want, want), (q, r, got)
    # no candidate at all: a full board without two equal neighbours
    full = sum((1 + (i + i // 4) % 2) << (4 * i) for i in range(16))
    assert (nt.moves_on_host([full])[0] == np.uint64(full)).all()
    assert _nt_action(full, (3, 3, 3, 3), 0) == -1 and common.greedy_scan_on_host((3, 3, 3, 3), None, (False,) * 4) == -1
