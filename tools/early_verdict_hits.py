"""How often a long launch's early look finds its verdict settled (PULSE_STOPRULE_OPT_EARLY_VERDICTS = 2): 40
episodes of a headline-like loop -- 65,536 tables of 10 seats, active players sampled 2..10, threshold 0.8, calls of up to 200
steps -- with the counting option on; prints the rule's stats and the settled share.  Counting delays the wavefronts that count
(section 6.0r8), so the share is a floor for the product's.
    python tools/early_verdict_hits.py [tables]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pulselib_amd.environments.Poker import PokerGPU  # noqa: E402
from pulselib_amd.stoprule import LaggedDoneCount  # noqa: E402

dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
env = PokerGPU(device=dev, agents=[], n_players=10, max_players=10, n_games=N, starting_bbs=100, max_bbs=1000, w1=.5, w2=.3, K=100, alpha=50, seed=20260401)
types = [3, 3, 2, 2, 4, 3, 1, 4, 5, 3]                       # config/pokerGPU.yaml's opponent mix (PULSE_AGENT_* codes)
rule = LaggedDoneCount(dev, N, 0.8, lag=1)
rule.set_option(LaggedDoneCount.OPT_EARLY_VERDICTS, 2)
acts = torch.zeros(N, dtype=torch.long, device=dev)
rng = np.random.default_rng(1)
gstep = 0
for e in range(40):
    rule.drain()
    env.reset(options={"active_players": int(rng.integers(2, 11)), "rotation": e})
    n, _ = env.rollout_until(types, acts, 5, 200, gstep, rule)
    gstep += n
torch.cuda.synchronize()
st = rule.stats()
print(f"40 episodes, {gstep} steps: {st}")
h, m = st["early_hits"], st["early_misses"]
print(f"early looks: {h} settled, {m} pending: {h / max(1, h + m):.3f} settled")
rule.close()
