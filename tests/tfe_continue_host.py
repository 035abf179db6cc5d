"""The host's side of the n-tuple network's games continued across rounds (csrc/tfe_ntuple_continue.hip), for
the tests: one round of continued games on the host -- the host's roll-out from `start` (tests/tfe_nt_host.py), then
continue_pick_on_host on its records -- with the bookkeeping a test keeps on its own beside the carries, and the chain of such rounds
under fixed weights.  A helper, not a test."""
import numpy as np

from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests.tfe_nt_host import nt_games_on_host, usable_on_host

WORDS = len(nt.FINISHED_SUMMARY) + nt.EVAL_BINS


class Carried:
    """What the pick launches carry from round to round -- start, carry_score, carry_moves, finished -- and beside them the test's own
    count of every game's moves so far: the sum of its segments' L - 1, kept without the mirror."""
    def __init__(self, n_games):
        self.start, self.score = np.zeros(n_games, dtype=np.uint64), np.zeros(n_games, dtype=np.int64)
        self.moves, self.finished = np.zeros(n_games, dtype=np.int32), [0] * WORDS
        self.so_far = np.zeros(n_games, dtype=np.int64)


def pick_on_host(c, games, max_steps, env_seed, board_id0):
    """continue_pick_on_host on the records `games` (keys, steps, lengths, total_score) under the carries of `c`, which it advances.
    Asserted here, on every call: the cut move made again gives the recorded afterstate (the mirror's own assertion), every board of
    the new `start` is usable and every other entry 0, finished and continued games are all the games, a finished game's length is
    the test's own sum of its segments' L - 1 plus the last L, and the carries of a finished game are 0.  Returns (the 24 words this
    pick adds, cut bool[B])."""
    B = len(games["lengths"])
    L = np.minimum(games["lengths"].astype(np.int64), max_steps)
    last = games["steps"][L - 1, np.arange(B)]
    start, score, moves, words = nt.continue_pick_on_host(games["keys"], games["steps"], games["lengths"], games["total_score"], max_steps, env_seed, board_id0,
                                                          c.score, c.moves)
    cut = start != 0
    assert usable_on_host(start[cut]).all() and words[0] + words[5] == B and words[5] == int(cut.sum())
    assert not (cut & ((last >> 7 != 0) | (L < max_steps))).any()          # a game that is over, or stopped early, is not continued
    assert words[1] == int((c.so_far[~cut] + L[~cut]).sum()) and words[6] == int((c.so_far[~cut] > 0).sum())
    assert sum(words[len(nt.FINISHED_SUMMARY):]) == words[0]
    c.so_far = np.where(cut, c.so_far + L - 1, 0)
    assert np.array_equal(moves, c.so_far) and not score[~cut].any()
    c.start, c.score, c.moves, c.finished = start, score, moves, nt.add_finished_on_host(c.finished, words)
    return words, cut


def round_on_host(c, n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round, **options):
    """One round of continued games: the host's roll-out from c.start (board_id0: the round's first board; `options`:
    nt_games_on_host's depth and backed), then pick_on_host.  Every board of c.start is usable, so the roll-out leaves `start` as it
    was.  Returns (the games, the words the pick adds, cut)."""
    games = nt_games_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round, start=c.start,
                             **options)
    assert np.array_equal(games["start_left"], c.start)
    words, cut = pick_on_host(c, games, max_steps, env_seed, board_id0)
    return games, words, cut
