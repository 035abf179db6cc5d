"""The host's side of the n-tuple network's expectimax search, one or two chance layers deep (csrc/tfe_ntuple_search.hip), for the
tests: packed boards from lists of nibbles, and the definition once more as plain recursive Python over one board -- an independent
statement of the search, not a roll-out (the games under it are tests/tfe_nt_host.py's).  A helper, not a test."""
import numpy as np

from pulselib_amd.agents import tfe_ntuple_td_gpu as nt


def key_of(nibbles) -> int:
    """the packed board of 16 nibbles (log2 tiles, 0 = empty), row-major"""
    assert len(nibbles) == 16 and all(0 <= int(x) <= 15 for x in nibbles)
    return sum(int(x) << (4 * i) for i, x in enumerate(nibbles))


# ------------------------------------------------------------------ the definition, one board at a time
def _chance_boards(after, key):
    """the chance boards of a board's candidate moves, as (a, slot, board)"""
    return [(a, 2 * cell + (k - 1), after[a] | k << (4 * cell)) for a in range(4) if after[a] != key for cell in range(16)
            if not (after[a] >> (4 * cell)) & 15 for k in (1, 2)]


def _tables(key, w, tuples, symmetric, layers):
    """(moves {board: (its four afterstates, their merge scores)}, values {afterstate: V}) of every board the tree of `key` reaches in
    `layers` chance layers: moves_on_host and value_on_host once per level, so that the arithmetic below only looks up"""
    moves, level = {}, [int(key)]
    for depth in range(layers + 1):
        new = sorted(set(level) - set(moves))
        if new:
            after, scores = nt.moves_on_host(np.array(new, dtype=np.uint64))
            moves.update((k, ([int(x) for x in after[i]], [int(x) for x in scores[i]])) for i, k in enumerate(new))
        level = [c for k in new for _, _, c in _chance_boards(moves[k][0], k)]
    leaves = sorted({b for after, _ in moves.values() for b in after})
    return moves, dict(zip(leaves, nt.value_on_host(np.array(leaves, dtype=np.uint64), w, tuples, symmetric).tolist()))


def _scalar_search(key, moves, values, gamma, layers):
    """(q: four np.float64, cand: four bools, terms: 4 x 32 np.float64) of one board by the definition of DESIGN.md section 13.4, in
    np.float64 scalars and explicit loops; at two layers it calls itself with one on every chance board."""
    after, scores = moves[key]
    q, cand, terms = [np.float64(0.0)] * 4, [after[a] != key for a in range(4)], [[np.float64(0.0)] * 32 for _ in range(4)]
    for a, slot, chance in _chance_boards(after, key):
        after2, scores2 = moves[chance]
        if layers == 2:
            x, c2, _ = _scalar_search(chance, moves, values, gamma, 1)
        else:
            c2 = [b != chance for b in after2]
            x = [np.float64(s.bit_length() - 1 if s > 0 else 0) + gamma * np.float64(values[b]) for b, s in zip(after2, scores2)]
        best, found = np.float64(0.0), False
        for m in range(4):
            if c2[m] and (not found or x[m] > best):
                best = x[m]
            found = found or c2[m]
        terms[a][slot] = np.float64(nt.TILE_ODDS[slot & 1]) * best
    for a in range(4):
        if cand[a]:
            level = list(terms[a])
            while len(level) > 1:
                level = [level[i] + level[i + 1] for i in range(0, len(level), 2)]
            n_empty = sum(1 for cell in range(16) if not (after[a] >> (4 * cell)) & 15)
            q[a] = np.float64(scores[a].bit_length() - 1 if scores[a] > 0 else 0) + gamma * (level[0] / np.float64(n_empty))
    return q, cand, terms


def scalar_search_on_host(key, w, tuples, symmetric, gamma, tie_seed, round, layers) -> dict:
    """q float64[4], candidates (bit a), action (-1: no candidate) and terms float64[4, 32] of one board: _scalar_search, then the
    roll-out's greedy scan written out -- the first candidate starts, a larger q replaces it, an equal q replaces it iff bit 31 of
    word a - 1 of Philox(tie_seed, key, round) is set."""
    moves, values = _tables(key, w, tuples, symmetric, layers)
    q, cand, terms = _scalar_search(int(key), moves, values, np.float64(gamma), layers)
    coins = nt.philox_many_on_host(tie_seed, np.array([key], dtype=np.uint64), int(round))[0]
    best = -1
    for a in range(4):
        if cand[a] and (best < 0 or q[a] > q[best] or (q[a] == q[best] and int(coins[a - 1]) >> 31)):
            best = a
    return dict(q=np.array(q, dtype=np.float64), candidates=sum(1 << a for a in range(4) if cand[a]), action=best,
                terms=np.array(terms, dtype=np.float64))
