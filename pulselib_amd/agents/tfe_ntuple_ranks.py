"""Rank-parallel rounds of the 2048 n-tuple agent (csrc/tfe_ntuple_exchange.hip): R ranks play disjoint games
of one round, each learns into its own accumulators, the accumulators are summed, and the apply launch runs replicated on every rank.

Why it is exact.  The learners never touch the weights: they add fixed-point integers into `acc` (and `acc_abs`), and integer adds
commute, so the sum of the ranks' accumulators is bit for bit the accumulator of one process that played all the games.  Every draw
of game g is keyed by its board's id, board_id0 + round * n_games_total + g, and the tie coin by the board and the round, so the rank
whose games begin at game0 plays exactly those games of the single process (tfe_ntuple_host.shard_round_board_id0).  The apply launch
on the merged accumulators therefore leaves the weights, E, A and tc_stats identical on all ranks and identical to the single process.

The exchange (`exchange_round`, once per round between learn and apply):
  1. every rank packs the cells it touched into its list (pulse_tfe_nt_acc_pack; header {found, written, 0, 0});
  2. the headers are all-gathered and READ ON THE HOST: the one host read a round costs in this mode.  Every rank sees the same
     headers, so every rank takes the same branch;
  3. if every rank's list held all it found (written == found): the lists, trimmed to the largest `found`, are all-gathered and every
     other rank's list is added into `acc` (pulse_tfe_nt_acc_unpack) -- the rank's own entries are there already; otherwise a dense
     all_reduce(SUM) of `acc` (and `acc_abs`), which is as exact.
Collectives follow environments/Poker/qnetwork.py: with gloo through host tensors (the one-device rehearsal), with any other backend
(nccl = RCCL) on device tensors; that path is written and has not run on a multi-GPU node.

`Shard` is what `agent.set_shard` hangs on the agent; `HostAccumulators` drives the same collective logic on numpy arrays with the
host's pack and unpack (tests/test_tfe_nt_ranks_cpu.py)."""
from __future__ import annotations

import datetime

import numpy as np

from .. import _native
from ..sharding import shard_tables
from .tfe_ntuple_host import ACC_LIST_ENTRY, ACC_LIST_HEADER, check_shard, pack_acc_on_host, shard_round_board_id0, unpack_acc_on_host

GROUP_TIMEOUT_S = 60                                                       # a dead rank ends the others instead of hanging them
SPARSE, DENSE = "sparse", "dense"


def init_ranks(backend, rank, world, init_method=None):
    """torch.distributed.init_process_group with the timeout of GROUP_TIMEOUT_S seconds; MASTER_ADDR / MASTER_PORT (or `init_method`)
    say where the ranks meet."""
    import torch.distributed as dist
    dist.init_process_group(backend, rank=int(rank), world_size=int(world), init_method=init_method,
                            timeout=datetime.timedelta(seconds=GROUP_TIMEOUT_S))


def group_of(group=None):
    """(group, world, rank): `group`, or the default group where torch.distributed is initialised, or (None, 1, 0): a world of one."""
    import torch.distributed as dist
    if group is None and not (dist.is_available() and dist.is_initialized()):
        return None, 1, 0
    return group, dist.get_world_size(group), dist.get_rank(group)


def shard_of(n_games_total, group=None):
    """(n_games, game0) of this rank: sharding.shard_tables over the group's ranks, so an uneven split gives the first ranks one more."""
    _, world, rank = group_of(group)
    return shard_tables(int(n_games_total), world, rank)


def _on_host(group) -> bool:
    import torch.distributed as dist
    return dist.get_backend(group) == "gloo"


def reduce_words(words, group, device=None, max_at=()):
    """`words` (ints) summed over the group's ranks, those at the positions `max_at` reduced with max; a world of one returns them as
    they are.  int64 on the host with gloo, on `device` otherwise."""
    import torch
    import torch.distributed as dist
    group, world, _ = group_of(group)
    words = [int(w) for w in words]
    if world == 1:
        return words
    t = torch.tensor(words, dtype=torch.int64, device="cpu" if _on_host(group) or device is None else device)
    total = t.clone()
    dist.all_reduce(total, group=group)
    if max_at:
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        total[list(max_at)] = t[list(max_at)]
    return total.cpu().tolist()


# ------------------------------------------------------------------ the two sides the collective logic drives
class HostAccumulators:
    """acc int64[W, 2] and acc_abs int64[W] or None as numpy arrays, exchanged in place with pack_acc_on_host and unpack_acc_on_host:
    exchange_round without a device."""

    def __init__(self, acc, acc_abs, capacity):
        self.acc, self.acc_abs, self.capacity = acc, acc_abs, int(capacity)
        self.added = self.refused = 0

    def pack(self):
        import torch
        entries = pack_acc_on_host(self.acc, self.acc_abs)
        written = min(len(entries), self.capacity)
        words = np.zeros(ACC_LIST_HEADER + ACC_LIST_ENTRY * self.capacity, dtype=np.int64)
        words[:2] = len(entries), written
        words[ACC_LIST_HEADER:ACC_LIST_HEADER + ACC_LIST_ENTRY * written] = entries[:written].reshape(-1)
        return torch.from_numpy(words)

    def unpack(self, words, capacity):
        words = words.cpu().numpy()
        written = int(words[1])
        if written > capacity:
            self.refused += capacity
            return
        added, refused = unpack_acc_on_host(self.acc, self.acc_abs, words[ACC_LIST_HEADER:ACC_LIST_HEADER + ACC_LIST_ENTRY * written])
        self.added, self.refused = self.added + added, self.refused + refused

    def dense(self):
        import torch
        return [torch.from_numpy(x) for x in (self.acc, self.acc_abs) if x is not None]


class DeviceAccumulators:
    """The agent's `acc` and `acc_abs` on the device, exchanged with pulse_tfe_nt_acc_pack / _unpack.  The list (int64[4 + 4 *
    capacity]) and the unpack counters (int64[2]) are allocated at first use."""

    def __init__(self, agent, capacity):
        self.agent, self.capacity = agent, int(capacity)
        self.list = self.stats = None

    def _struct(self, words, capacity):
        import torch
        a = self.agent
        if self.stats is None:
            self.stats = torch.zeros(2, dtype=torch.int64, device=a.device)
        o = _native.TfeNtAccList()
        o.n_entries, o.acc, o.acc_abs = a.total_weights, a.acc.data_ptr(), None if a.acc_abs is None else a.acc_abs.data_ptr()
        o.capacity, o.list, o.stats = capacity, words.data_ptr(), self.stats.data_ptr()
        return o

    def pack(self):
        import torch
        if self.list is None:
            self.list = torch.zeros(ACC_LIST_HEADER + ACC_LIST_ENTRY * self.capacity, dtype=torch.int64, device=self.agent.device)
        self.agent._launch("pulse_tfe_nt_acc_pack", self._struct(self.list, self.capacity))
        return self.list

    def unpack(self, words, capacity):
        self.agent._launch("pulse_tfe_nt_acc_unpack", self._struct(words, capacity))

    def dense(self):
        return [x for x in (self.agent.acc, self.agent.acc_abs) if x is not None]


def exchange_round(side, group) -> dict:
    """One round's exchange over `group` on `side` (HostAccumulators or DeviceAccumulators), steps 1 to 3 of the module's docstring.
    Afterwards every rank's accumulators hold the sum over the ranks.  Returns dict(path, entries, bytes): SPARSE or DENSE, the
    entries every rank found, and the bytes this rank's collectives gathered or reduced.  A world of one packs (the entries are
    counted) and moves nothing."""
    import torch
    import torch.distributed as dist
    group, world, rank = group_of(group)
    words = side.pack()
    if world == 1:
        found = int(words[0].item())                                        # (the same one host read)
        return dict(path=SPARSE if found <= side.capacity else DENSE, entries=[found], bytes=0)
    on_host = _on_host(group)
    wire = (lambda t: t.cpu()) if on_host else (lambda t: t)
    head = wire(words[:ACC_LIST_HEADER]).contiguous()
    heads = torch.empty(world * ACC_LIST_HEADER, dtype=torch.int64, device=head.device)
    dist.all_gather_into_tensor(heads, head, group=group)
    heads = heads.view(world, ACC_LIST_HEADER).cpu().tolist()                                            # the round's one host read
    entries, moved = [h[0] for h in heads], 8 * ACC_LIST_HEADER * world
    if all(h[1] == h[0] for h in heads):                                    # every list holds all its rank found
        most = max(entries)
        if most:
            n = ACC_LIST_HEADER + ACC_LIST_ENTRY * most
            mine = words[:n]
            if mine.numel() < n:                                            # (a rank whose own capacity is below another rank's count)
                mine = torch.zeros(n, dtype=torch.int64, device=words.device)
                mine[:words.numel()] = words
            mine = wire(mine).contiguous()
            lists = torch.empty(world * n, dtype=torch.int64, device=mine.device)
            dist.all_gather_into_tensor(lists, mine, group=group)
            lists = lists.to(words.device).view(world, n)                   # (a row is a list: its header, then `most` entries; 32 (1 + most) bytes)
            for r in range(world):
                if r != rank and entries[r]:
                    side.unpack(lists[r], most)
            moved += 8 * n * world
        return dict(path=SPARSE, entries=entries, bytes=moved)
    for t in side.dense():
        if on_host:
            total = t.cpu()
            dist.all_reduce(total, group=group)
            t.copy_(total)
        else:
            dist.all_reduce(t, group=group)
        moved += 8 * t.numel()
    return dict(path=DENSE, entries=entries, bytes=moved)


# ------------------------------------------------------------------ what set_shard hangs on the agent
class Shard:
    """A rank's share of the agent's rounds: the job's games, the rank's first, the group, the device side of the exchange and the
    rounds' records."""

    def __init__(self, agent, n_games_total, game0, group=None, exchange_capacity=None):
        self.n_games_total, self.game0, _ = check_shard(n_games_total, game0, agent.n_games)
        self.group = group
        largest = min(agent.total_weights, agent.n_games * agent.max_steps * agent.n_features)       # a round cannot touch more cells
        if exchange_capacity is None:
            exchange_capacity = largest
        if isinstance(exchange_capacity, bool) or not isinstance(exchange_capacity, (int, np.integer)) or int(exchange_capacity) < 1:
            raise ValueError("exchange_capacity must be None or a positive int")
        self.side = DeviceAccumulators(agent, min(int(exchange_capacity), largest))
        self.device, self.rounds = agent.device, []

    def round_board_id0(self, board_id0, round) -> int:
        return shard_round_board_id0(board_id0, round, self.n_games_total, self.game0)

    def exchange(self, round) -> dict:
        rec = dict(exchange_round(self.side, self.group), round=int(round))
        self.rounds.append(rec)
        return rec

    def reduce(self, words, max_at=()):
        return reduce_words(words, self.group, self.device, max_at)

    def eval_shard(self, n_games_total, board_id0):
        """(n_games, board_id0) of this rank's share of an evaluation of `n_games_total` games that begin at `board_id0`"""
        n, g0 = shard_of(n_games_total, self.group)
        return n, shard_round_board_id0(board_id0, 0, n_games_total, g0) & 0xFFFFFFFFFFFFFFFF

    def summary(self, clear=True) -> dict:
        """dict(rounds, added, refused): per round since the last clear its record (round, path, entries per rank, bytes), and the
        entries the unpack launches added and refused (synchronises)."""
        stats = [0, 0] if self.side.stats is None else self.side.stats.cpu().tolist()
        out = dict(rounds=list(self.rounds), added=stats[0], refused=stats[1])
        if clear:
            self.rounds.clear()
            if self.side.stats is not None:
                self.side.stats.zero_()
        return out
