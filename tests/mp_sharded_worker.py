"""Worker of the three-rank persistent-sweep tests of tests/test_gpu_sharded.py (ranks under torch.distributed.run, all on device 0,
process group over gloo): the row-sharded persistent sweep with its ranks in DIFFERENT processes, so that every rank's launches
get hardware queues of their own. Reads the design from <dir>/design.npz, connects the ranks' exchange buffers
(myfm_amd.distributed.connect_peers: IPC handles; MYFM_PEER_MODEL=1: the peers' w / V as well), runs three iterations and writes
what the test checks to <dir>/rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import scipy.sparse as sps
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ["MYFM_AMD_DEVICE"] = "0"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from myfm_amd import _capi, _myfm
    from myfm_amd import distributed as D

    out_dir = sys.argv[1]
    d = np.load(os.path.join(out_dir, "design.npz"))
    X = sps.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=tuple(int(v) for v in d["shape"]))
    y, gi, cuts, K = d["y"], d["gi"], d["cuts"], int(d["K"])
    n = X.shape[0]
    lo, hi = int(cuts[rank]), int(cuts[rank + 1])
    b = _myfm.ConfigBuilder()
    b.set_alpha_0(1.0).set_beta_0(1.0).set_gamma_0(1.0).set_mu_0(0.0).set_reg_0(1.0)
    b.set_group_index([int(g) for g in gi]).set_n_iter(8).set_n_kept_samples(0).set_task_type(_myfm.TaskType.REGRESSION)
    ar = D.TorchAllReduce()
    s = _myfm.GibbsSession(K, 0.1, X[lo:hi], [], y[lo:hi], 42, b.build(), allreduce=ar, n_total_rows=n, row_offset=lo,
                           stream=ar.stream_ptr, main_levels=_capi.column_levels(X)[0], shard_rank=rank, shard_world=world)
    pending, sum_p, flag_p, sum_b = s.peer_info()[:4]
    info_ok = bool(pending and sum_p and flag_p and sum_b > 0)
    flags_before = s.plan_flags()  # (not live before every rank knows every rank's buffers)
    verdicts = [None] * world
    dist.all_gather_object(verdicts, bool(pending))
    live = D.connect_peers(s)
    flags = s.plan_flags()
    calls0 = s.comm_stats()[0]
    for _ in range(3):
        s.step()
    s.synchronize()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), pending=bool(pending), info_ok=info_ok, verdicts=np.array(verdicts),
             live=bool(live), flags_before=flags_before, flags=flags, flags_after=s.plan_flags(), calls=s.comm_stats()[0] - calls0,
             w0=s.fm.w0, w=np.asarray(s.fm.w), V=np.asarray(s.fm.V), e=s.residual(), lo=lo)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
