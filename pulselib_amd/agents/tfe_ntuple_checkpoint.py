"""The 2048 n-tuple network's checkpoint file: an .npz of plain arrays that holds the non-zero weights, the tuples and the run's scalars,
and by format version `lam`, the temporal-coherence sums E and A (13.3) and the stage tiles (13.9).  How rounds
are played, learnt and evaluated -- search depth, backed targets, restarts, continuation -- is in no file.  numpy alone: no device."""
from __future__ import annotations

import numpy as np

from .tfe_ntuple_host import MAX_LEN, check_stage_tiles, tuple_offsets, with_stages

CHECKPOINT_VERSION = 1                                                                        # what an agent with lam == 0 writes
CHECKPOINT_VERSION_LAMBDA = 2                                                                 # ... and with lam != 0: version 1's arrays and `lam`
CHECKPOINT_VERSION_TC = 4                                                                     # ... and with tc: version 2's and tc_index / tc_e / tc_a (3 is not a format)
CHECKPOINT_VERSION_STAGED = 5                                                                 # ... and with stage_tiles: version 2's or 4's arrays over S * W weights and `stage_tiles`
CHECKPOINT_SCALARS = ("symmetric", "gamma", "epsilon", "alpha", "max_steps", "seed", "board_id0", "round", "n_games")


def write_checkpoint(path, weights, tuples, lam=0.0, tc=None, stage_tiles=(), **scalars) -> None:
    """The network as an .npz of plain arrays (np.savez, no pickles): the non-zero weights as index int64[m] (ascending) and value
    float32[m], the tuples as tuple_len int64[n_tuples] and tuple_cells int64[n_tuples, 6] (-1 beyond a tuple's length), the scalars of
    CHECKPOINT_SCALARS as 0-d arrays and `version`.  lam == 0 writes exactly that, as version 1; any other `lam` adds a 0-d float64
    `lam` and writes version 2.  tc = (E, A), float64[n_weights] each, writes version 4: version 2's arrays with `lam` whatever its
    value, tc_index int64[m'] (ascending: the weights whose E or A is not +0.0 by bit pattern) and tc_e / tc_a float64[m'].
    stage_tiles other than () writes version 5: version 2's arrays (with `lam` whatever its value) or, with tc, version 4's, every index
    over the S * W weights of the staged network, and stage_tiles int64[S - 1].  `path` is written as given."""
    if sorted(scalars) != sorted(CHECKPOINT_SCALARS):
        raise ValueError(f"a checkpoint holds exactly the scalars {CHECKPOINT_SCALARS}")
    weights = np.asarray(weights, dtype=np.float32).reshape(-1)
    index = np.flatnonzero(weights.view(np.uint32) != 0)                   # by bit pattern: what is not +0.0 is kept
    cells = np.full((len(tuples), MAX_LEN), -1, dtype=np.int64)
    for i, t in enumerate(tuples):
        cells[i, :len(t)] = t
    dtypes = dict(gamma=np.float64, epsilon=np.float64, alpha=np.float64, seed=np.uint64, board_id0=np.uint64)
    arrays = {k: np.array(scalars[k], dtype=dtypes.get(k, np.int64)) for k in CHECKPOINT_SCALARS}
    version, stage_tiles = CHECKPOINT_VERSION, check_stage_tiles(stage_tiles)
    if float(lam) != 0.0 or tc is not None or stage_tiles:
        arrays["lam"], version = np.array(lam, dtype=np.float64), CHECKPOINT_VERSION_LAMBDA
    if tc is not None:
        E, A = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in tc)
        if E.shape != weights.shape or A.shape != weights.shape:
            raise ValueError("tc = (E, A), one float64 per weight each")
        at = np.flatnonzero((E.view(np.uint64) != 0) | (A.view(np.uint64) != 0))
        arrays.update(tc_index=at.astype(np.int64), tc_e=E[at], tc_a=A[at])
        version = CHECKPOINT_VERSION_TC
    if stage_tiles:
        arrays["stage_tiles"], version = np.array(stage_tiles, dtype=np.int64), CHECKPOINT_VERSION_STAGED
    with open(path, "wb") as fh:
        np.savez(fh, version=np.array(version, dtype=np.int64), index=index.astype(np.int64), value=weights[index],
                 tuple_len=np.array([len(t) for t in tuples], dtype=np.int64), tuple_cells=cells, **arrays)


def read_checkpoint(path) -> dict:
    """What write_checkpoint wrote (np.load with allow_pickle=False), version 1, 2, 4 or 5: `tuples`, `index`, `value`, `n_weights`, the
    scalars as Python numbers, `lam` (0.0 for version 1), `tc` (False for versions 1 and 2) and `stage_tiles` (() below version 5); with
    tc also `tc_index`, `tc_e` and `tc_a`.  For version 5 `n_weights` is S * W, all stages', and `tc` says whether the file holds the tc
    arrays.  ValueError for another format version, a missing array, tuples or stage tiles the library would refuse or an index outside
    the network."""
    with np.load(path, allow_pickle=False) as f:
        missing = [k for k in ("version", "index", "value", "tuple_len", "tuple_cells") + CHECKPOINT_SCALARS if k not in f.files]
        if missing:
            raise ValueError(f"{path}: not an n-tuple network checkpoint (no {missing})")
        version = int(f["version"])
        if version not in (CHECKPOINT_VERSION, CHECKPOINT_VERSION_LAMBDA, CHECKPOINT_VERSION_TC, CHECKPOINT_VERSION_STAGED):
            raise ValueError(f"{path}: format version {version}, this package reads {CHECKPOINT_VERSION}, {CHECKPOINT_VERSION_LAMBDA}, "
                             f"{CHECKPOINT_VERSION_TC} and {CHECKPOINT_VERSION_STAGED}")
        if version == CHECKPOINT_VERSION_STAGED and "stage_tiles" not in f.files:
            raise ValueError(f"{path}: format version {version} is a staged network's, and the file holds no stage_tiles")
        tc_names = ("tc_index", "tc_e", "tc_a")
        has_tc = version == CHECKPOINT_VERSION_TC or (version == CHECKPOINT_VERSION_STAGED and any(k in f.files for k in tc_names))
        more = ("lam",) * (version != CHECKPOINT_VERSION) + tc_names * has_tc
        if version == CHECKPOINT_VERSION_STAGED:
            more += ("stage_tiles",)
        missing = [k for k in more if k not in f.files]
        if missing:
            raise ValueError(f"{path}: not an n-tuple network checkpoint (no {missing})")
        out = {k: (float(f[k]) if k in ("gamma", "epsilon", "alpha") else int(f[k])) for k in CHECKPOINT_SCALARS}
        out["lam"] = float(f["lam"]) if "lam" in more else 0.0
        out["tc"] = has_tc
        index, value, lens, cells = f["index"], f["value"], f["tuple_len"], f["tuple_cells"]
        tc_arrays = [f[k] for k in tc_names * has_tc]
        out["stage_tiles"] = check_stage_tiles(f["stage_tiles"].tolist()) if version == CHECKPOINT_VERSION_STAGED else ()
    if version == CHECKPOINT_VERSION_STAGED and not out["stage_tiles"]:
        raise ValueError(f"{path}: a version {CHECKPOINT_VERSION_STAGED} checkpoint holds at least one stage tile")
    out["symmetric"] = bool(out["symmetric"])
    out["tuples"] = with_stages([cells[i, :int(n)].tolist() for i, n in enumerate(lens.tolist())], out["stage_tiles"])
    out["n_weights"] = tuple_offsets(out["tuples"])[1] * (len(out["stage_tiles"]) + 1)
    def check_sparse(name, index, others, dtype, shapes):
        """index int64[m], strictly ascending inside the network, and `others` of `dtype` in its shape (ValueError)"""
        if index.dtype != np.int64 or index.ndim != 1 or any(x.dtype != dtype or x.shape != index.shape for x in others):
            raise ValueError(f"{path}: {shapes}")
        if len(index) and (int(index[0]) < 0 or int(index[-1]) >= out["n_weights"] or not bool((index[1:] > index[:-1]).all())):
            raise ValueError(f"{path}: {name} must be strictly ascending inside the network's {out['n_weights']} weights")
    check_sparse("index", index, [value], np.float32, "index must be int64[m] and value float32[m]")
    out["index"], out["value"] = index, value
    if out["tc"]:
        check_sparse("tc_index", tc_arrays[0], tc_arrays[1:], np.float64, "tc_index must be int64[m] and tc_e / tc_a float64[m]")
        out["tc_index"], out["tc_e"], out["tc_a"] = tc_arrays
    return out


def coherence_of_checkpoint(f: dict):
    """(E, A), float64[n_weights] each, of a version-4 read_checkpoint dict."""
    E, A = np.zeros(f["n_weights"], dtype=np.float64), np.zeros(f["n_weights"], dtype=np.float64)
    E[f["tc_index"]], A[f["tc_index"]] = f["tc_e"], f["tc_a"]
    return E, A


def weights_of_checkpoint(f: dict) -> np.ndarray:
    """float32[n_weights] of a read_checkpoint dict."""
    w = np.zeros(f["n_weights"], dtype=np.float32)
    w[f["index"]] = f["value"]
    return w
