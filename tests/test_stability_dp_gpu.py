"""Training-stability metrics of the data-parallel learner: two ranks on one device (gloo, as tests/test_qnetwork_dp_gpu.py)
all-reduce the per-call totals ({rows, sum |td|, sum Q} with SUM, {-min Q, max Q} with MAX) before pulse_qnet_train_apply
normalises them: the job-wide per-call block equals that of one process trained on the concatenated batch."""
import os

import numpy as np
import pytest
import torch

from tests import test_qnetwork_dp_gpu as DP

pytestmark = pytest.mark.gpu


def _steps(q, lo, hi, n_total):
    q.enable_stability_metrics()
    blocks = []
    for it in range(3):
        b = DP._batch(n_total, 500 + it)
        dev = {k: torch.from_numpy(x[lo:hi]).to("cuda:0") for k, x in b.items()}
        q.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"],
                            step_counter=70 + it)
        blocks.append(q.stability_step().cpu().numpy().copy())
    acc = q.stability_episode().cpu().numpy().copy()
    return np.stack(blocks), acc


def _worker(rank, world, port, golden_path, n_total, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        half = n_total // world
        q = DP._make(golden_path, table_id0=rank * half)
        out[rank] = _steps(q, rank * half, (rank + 1) * half, n_total)
    finally:
        dist.destroy_process_group()


def test_two_ranks_report_the_job_wide_metrics(golden_dir):
    import torch.multiprocessing as mp
    n_total, world = 6000, 2
    path = str(golden_dir / "qnetwork.npz")
    want, want_acc = _steps(DP._make(path, 0), 0, n_total, n_total)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, DP._free_port(), path, n_total, out), nprocs=world, join=True)
    for r in range(world):
        got, acc = out[r]
        assert np.array_equal(got[:, 0], want[:, 0]), f"rank {r}: job-wide row counts"
        assert np.array_equal(got[:, 3:5], want[:, 3:5]) or np.allclose(got[:, 3:5], want[:, 3:5], rtol=0, atol=1e-5), f"rank {r}: min / max Q"
        # sums in another order (two partial sums + an all-reduce); the parameters themselves differ by <= 1e-5 (the DP test)
        np.testing.assert_allclose(got[:, 1:3], want[:, 1:3], rtol=1e-4, atol=1e-5, err_msg=f"rank {r}: mean |td|, mean Q")
        np.testing.assert_allclose(got[:, 5], want[:, 5], rtol=1e-4, err_msg=f"rank {r}: gradient norm")
        np.testing.assert_array_equal(got[:, 6], want[:, 6])
        np.testing.assert_allclose(got[:, 7], want[:, 7], rtol=1e-4, err_msg=f"rank {r}: loss")
        assert acc[0] == want_acc[0] == 3
    np.testing.assert_array_equal(out[0][0], out[1][0])                      # every rank holds the same block
