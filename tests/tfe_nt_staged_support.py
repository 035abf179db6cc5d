"""What the two test files of the 2048 n-tuple network's weight sets by tile stage share (tests/test_tfe_nt_staged_*.py; DESIGN.md
section 13.9): the stage tiles of the tests, the stages struct, weights with a slice of its own per stage, boards on either side of
every threshold, and the count of adds per stage.  The stages travel to the host mirrors on `tuples` (with_stages), so
tests/tfe_host.py, tests/tfe_nt_host.py, tests/tfe_search_host.py and tests/tfe_nt_support.py serve staged networks as they are.
A helper, not a test."""
import functools

import numpy as np

from tests.tfe_nt_support import CRAFTED, MORE, TUPLES, nt
from tests.tfe_search_host import key_of

STAGE_TILES = (8, 32)                                                      # nibbles 3 and 5: a game from reset crosses both in its first few dozen moves
UNREACHED = 16384                                                          # a tile no game of the tests' lengths reaches


def stages_struct(tiles=STAGE_TILES, **kw):
    """PulseTfeNtStages of `tiles`, then `kw` over its fields (threshold: a list of four bytes)"""
    from pulselib_amd import _native
    st = _native.TfeNtStages()
    st.n_stages = len(tiles) + 1
    for i, tile in enumerate(tiles):
        st.threshold[i] = int(tile).bit_length() - 1
    for k, v in kw.items():
        if k == "threshold":
            for i, x in enumerate(v):
                st.threshold[i] = x
        else:
            setattr(st, k, v)
    return st


def staged(tuples=TUPLES, tiles=STAGE_TILES):
    return nt().with_stages(tuples, tiles)


@functools.lru_cache(maxsize=None)
def _staged_weights(tuples, n_stages, scale_divisor):
    n = nt().tuple_offsets(tuples)[1]
    w = (np.random.default_rng(11).standard_normal(n_stages * n) * 4).astype(np.float32) / np.float32(scale_divisor)
    w.setflags(write=False)
    return w


def staged_weights(tuples=TUPLES, n_stages=len(STAGE_TILES) + 1, divisor=1):
    """float32[n_stages * W], read-only, made once: seeded normal of scale 4 / divisor, every stage's slice different"""
    return _staged_weights(tuple(tuple(t) for t in tuples), n_stages, divisor)


def boards(tiles=STAGE_TILES):
    """uint64[N]: tfe_nt_support's crafted boards and, for every threshold nibble n, live boards whose largest nibble is n - 1 and n --
    one of them with its largest tile in the upper word -- and a board one merge below the threshold, whose afterstates straddle it"""
    out = [key_of(v) for v in list(CRAFTED.values()) + list(MORE.values())]
    for tile in tiles:
        n = int(tile).bit_length() - 1
        out.append(key_of([n - 1, 1, 0, 0] + [0] * 12))                    # below
        out.append(key_of([n, 1, 0, 0] + [0] * 12))                        # at
        out.append(key_of([0] * 12 + [0, 1, 2, n]))                        # at, in the upper word
        out.append(key_of([n - 1, n - 1, 1, 0] + [0] * 8 + [0, 1, 2, 0]))  # a merge to the left or the right reaches it, up and down merge nothing
    return np.array(out, dtype=np.uint64)


def adds_per_stage(acc, n_stages):
    """the adds every stage's slice of acc int64[S * W, 2] received"""
    return [int(x[:, 1].sum()) for x in np.asarray(acc).reshape(n_stages, -1, 2)]
