"""The host's side of the tabular Q-learner (csrc/qtable.hip, agents/qlearning.py) with private tables, for the tests: B copies of the
reference agent, one dict {state key: float64[4]} per board, on the oracle's environment (oracle.tfe_reset / oracle.tfe_step) and the
oracle's two scalar helpers -- plus what a region of `slots` entries adds to the reference, stated once:
  (a) a state that finds no room (the region holds `slots` other keys) acts by (w[2] * 4) >> 32 and has no row this step;
  (b) a state s' that finds no room counts as max q(s') = 0;
  (c) a board without a row for s changes nothing.
A private region has at most 4,096 slots, the probe limit, so an insert fails exactly when the region holds `slots` keys: no hash here.
The key is the device's: 4 bits of min(log2 tile, 15) per cell, cell 0 in the low nibble -- lossy for the tiles 1 and 3, for negative
tiles and for tiles >= 65,536, on purpose.  Every path is counted, so that a test can tell what it exercised.  A helper, not a test."""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents.tfe_common import philox_many_on_host       # (the package's vectorised Philox, held to the oracle's by its own tests)

COUNTERS = ("terminal", "terminal_after_done", "no_room_s", "no_room_next")


def pack_board(b):
    """the state key of one board (tfe_table_device.h: pack_cells)"""
    key = 0
    for i, v in enumerate(np.asarray(b).reshape(-1).tolist()):
        key |= (min(int(v).bit_length() - 1, 15) if v > 0 else 0) << (4 * i)
    return key


def uniform53(w):
    """p of the epsilon branch: 53 bits of the Philox words 0 and 1"""
    return float(((int(w[0]) << 21) ^ (int(w[1]) >> 11)) * (1.0 / 9007199254740992.0))


class QLearningHost:
    """B private learners.  slots None: a dict without bound (the reference); else a region's capacity.  `boards`, `score`, `rewards`,
    `dones`, `actions` hold the last step's results; `tables[g]` the rows of board g; `counts` the paths taken so far."""

    def __init__(self, n_boards, n, slots, alpha, gamma, epsilon, env_seed, agent_seed, board_id0=0):
        self.B, self.n, self.slots = int(n_boards), int(n), slots
        self.alpha, self.gamma, self.epsilon = float(alpha), float(gamma), float(epsilon)
        self.env_seed, self.agent_seed, self.board_id0 = int(env_seed), int(agent_seed), int(board_id0)
        self.boards = np.zeros((self.B, n, n), dtype=np.int32)
        self.score = np.zeros(self.B, dtype=np.int64)
        self.rewards, self.dones = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.uint8)
        self.actions = np.zeros(self.B, dtype=np.int64)
        self.tables = [dict() for _ in range(self.B)]
        self.ever_done = np.zeros(self.B, dtype=bool)
        self.counts = dict.fromkeys(COUNTERS, 0)
        self.env_step = 0
        self._lib = orc.lib()
        orc.tfe_reset(self.boards, self.score, n, self.env_seed, self.board_id0)

    def row(self, g, key):
        """board g's row of `key`, inserted if absent and there is room; None: no room"""
        assert key != 0                                   # (0 marks a free entry on the device; no board with a tile >= 2 packs to it)
        table = self.tables[g]
        q = table.get(key)
        if q is None and (self.slots is None or len(table) < self.slots):
            q = table[key] = np.zeros(4, dtype=np.float64)
        return q

    def step(self, agent_step):
        """One step of every board: select under the agent's draw of `agent_step`, the environment's next step, the update."""
        lib, rows = self._lib, [None] * self.B
        for g in range(self.B):
            w = orc.philox4x32(self.agent_seed, self.board_id0 + g, agent_step)
            q = rows[g] = self.row(g, pack_board(self.boards[g]))
            if q is None:                                 # (a)
                self.actions[g] = (int(w[2]) * 4) >> 32
                continue
            self.actions[g] = lib.oracle_select_action_epsilon_greedy(q.ctypes.data_as(C.c_void_p), 4, C.c_double(self.epsilon),
                                                                      C.c_double(uniform53(w)), C.c_uint32(int(w[2])))
        self.env_step += 1
        orc.tfe_step(self.boards, self.score, self.actions, self.rewards, self.dones, self.n, self.env_seed, self.env_step, self.board_id0)
        zeros = np.zeros(4, dtype=np.float64)
        for g in range(self.B):
            cur, done = rows[g], int(self.dones[g])
            if cur is None:                               # (c)
                self.counts["no_room_s"] += 1
                continue
            nxt = self.row(g, pack_board(self.boards[g]))
            if nxt is None:                               # (b)
                self.counts["no_room_next"] += 1
                nxt = zeros
            self.counts["terminal"] += done
            self.counts["terminal_after_done"] += done and bool(self.ever_done[g])
            lib.oracle_update_q_entry(cur.ctypes.data_as(C.c_void_p), int(self.actions[g]), nxt.ctypes.data_as(C.c_void_p), 4,
                                      C.c_double(self.alpha), C.c_double(float(self.rewards[g])), C.c_double(self.gamma), done)
        self.ever_done |= self.dones != 0
        return self.actions

    def has_row(self):
        """bool[B]: the board a game is on now has a row in its table"""
        return np.array([pack_board(self.boards[g]) in self.tables[g] for g in range(self.B)])

    def summary(self):
        """the counters: the paths of `counts`, the boards ever done, the full regions, the rows with a non-zero value"""
        full = 0 if self.slots is None else sum(len(t) == self.slots for t in self.tables)
        return dict(self.counts, boards_done=int(self.ever_done.sum()), full_regions=full, rows=sum(len(t) for t in self.tables),
                    nonzero_rows=sum(bool(np.any(q != 0.0)) for t in self.tables for q in t.values()))


SHARED_SEED = 1                                   # the agent's seed in the shared table's tests
# (boards, alpha) at which one lost update of a contended cell moves it by > 10^4 tolerances (tests/test_qtable_cpu.py)
SHARED_SENSITIVE = ((700, 2.0 ** -10), (1300, 2.0 ** -10), (66000, 2.0 ** -16))


def combined(q0, target, k, alpha):
    """A shared table's cell after k transitions of one launch: each with `target` (the mean of their targets), one after another --
    q0 + (1 - (1 - alpha)^k) (target - q0), the header of csrc/qtable.hip"""
    return q0 + (1.0 - (1.0 - alpha) ** k) * (target - q0)


def combined_tolerance(k, target, q0):
    """What k updates may differ by in float64: each is three rounded operations (t - q, alpha *, q +) on values no larger than
    max(|t|, |q0|), and a later update multiplies an earlier one's error by (1 - alpha) < 1, so the errors add up to at most
    3 k 2^-53 max(|t|, |q0|); a few units more for the pow of the combined form and of `combined` itself: 4 k 2^-53 max(|t|, |q0|)."""
    return 4.0 * k * 2.0 ** -53 * max(abs(target), abs(q0))


def random_actions(seed, board_id0, n_boards, step):
    """int64[B]: what every board takes where epsilon is 1, (w[2] * 4) >> 32 of its Philox draw"""
    words = philox_many_on_host(seed, np.arange(n_boards, dtype=np.uint64) + np.uint64(board_id0), step)
    return ((words[:, 2].astype(np.uint64) * np.uint64(4)) >> np.uint64(32)).astype(np.int64)


def play(host, steps, first_step=0, between=None):
    """`steps` steps of `host` with the agent's draws first_step, first_step + 1, ...; between(t, host), if given, runs after step t
    (boards changed behind the agent's back).  Returns the per-step records: actions int64[steps, B], boards int32[steps, B, n, n],
    rewards, dones, scores, and has_row bool[steps, B] of the boards the games are then on."""
    out = dict(actions=[], boards=[], rewards=[], dones=[], scores=[], has_row=[])
    for t in range(first_step, first_step + steps):
        host.step(t)
        for k, v in zip(out, (host.actions, host.boards, host.rewards, host.dones, host.score, host.has_row())):
            out[k].append(v.copy())
        if between is not None:
            between(t, host)
    return {k: np.stack(v) for k, v in out.items()}


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share
CFG = dict(alpha=0.1, gamma=0.99, epsilon=0.1, env_seed=77, agent_seed=991)
UNUSUAL = (1, 3, 6, -2, 32768, 65536, 2 ** 20, 12, 5)      # tiles the packed 4 x 4 form cannot hold
LONE, MERGER = 64 + 37, 256 + 64 + 10                      # 4 x 4 case: wavefront 1's one unusual board; the board that merges 16,384s
FLIP_AFTER = 31                                            # 3 x 3 "flipped": every second board is turned over after this step
CASES = {                                                  # name: (n, boards, slots per board, steps, first board id)
    "3x3-room": (3, 200, 256, 64, 0),                      # 200 boards: three wavefronts and eight lanes
    "3x3-full": (3, 200, 16, 64, 0),
    "3x3-full-id1000": (3, 200, 16, 64, 1000),
    "3x3-flipped": (3, 200, 256, 64, 0),
    "4x4-unusual": (4, 512, 64, 12, 0),
}


def unusual_boards():
    """int32[512, 4, 4] of the 4 x 4 case: random ordinary boards (tiles 2 .. 2,048); wavefront 1 holds ONE board with an unusual cell
    (LONE), wavefront 3 one in every board, all kinds in turn; MERGER, in the otherwise ordinary wavefront 5, is the board whose move
    to the left merges 16,384 + 16,384 twice: it holds 32,768 afterwards, which the packed form cannot."""
    rng = np.random.default_rng(4)
    boards = ((2 ** rng.integers(1, 12, (512, 4, 4))) * (rng.random((512, 4, 4)) < 0.7)).astype(np.int32)
    boards[:, 0, 0] = np.maximum(boards[:, 0, 0], 2)       # (no board packs to the key 0)
    for i, g in enumerate([LONE] + list(range(192, 256))):
        r, c = rng.integers(0, 4, 2)
        boards[g, r, c] = UNUSUAL[i % len(UNUSUAL)]
    boards[MERGER] = np.array([[16384] * 4, [2, 2, 4, 4], [0] * 4, [8192, 8192, 0, 4096]])
    return boards


def flip_boards(t, host):
    if t == FLIP_AFTER:
        host.boards[::2] = host.boards[::2, ::-1].copy()


_RUNS = {}


def run_case(name):
    """(the host after the case's steps, play()'s records); played once, shared and not to be changed.  "4x4-unusual" starts from
    unusual_boards() with q[0] = 1 in MERGER's first row, so that its first move is to the left unless the epsilon branch draws."""
    if name not in _RUNS:
        n, B, slots, steps, board_id0 = CASES[name]
        host = QLearningHost(B, n, slots, board_id0=board_id0, **CFG)
        if name == "4x4-unusual":
            host.boards[:] = unusual_boards()
            host.row(MERGER, pack_board(host.boards[MERGER]))[0] = 1.0
        _RUNS[name] = host, play(host, steps, between=flip_boards if name == "3x3-flipped" else None)
    return _RUNS[name]
