"""Sharded evaluation on the real engine, one process per rank: gathered blocks and all-reduced normal-equation
products must equal the single-process results, and the sharded device LM must land on the same cost.

Two launches of the SAME worker:
  * gloo, both ranks on the one GPU of the test box (control plane through the host) — always runs;
  * nccl (= RCCL over xGMI), one GPU per rank, blocks gathered and products reduced on the device — runs wherever
    ``torch.cuda.device_count() >= 2`` (auto-skipped on a one-GPU box), so the first multi-GPU test box proves that RCCL
    has seen N ranks without anybody editing this file."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _Camset:
    def __init__(self, n):
        self.names = [f"cam_{i}" for i in range(n)]

    def get_names(self):
        return list(self.names)

    def get_n_cams(self):
        return len(self.names)


class _Target:
    def __init__(self, pts):
        self.point_data = np.asarray(pts)[None]


def _worker(rank, world, port, out_dir, backend="gloo"):
    sys.path.insert(0, str(REPO))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver only supports dmabuf IPC (RCCL needs it)
    rccl = backend == "nccl"
    device = rank if rccl else 0                 # RCCL: one GPU per rank; gloo: the ranks share GPU 0
    torch.cuda.set_device(device)
    if rccl:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pycamset_amd import handlers, sharding, synthetic
        from pycamset_amd.detections import TargetDetection
        from pycamset_amd.device_solver import JacobianOperator, lm_solve
        from pycamset_amd.engine import Engine

        rig = synthetic.make_rig("ring-8-small", 8, 12, synthetic.charuco_points(9, 8.0), seed=21, visibility=0.8)
        det = rig.detections
        counts = (rig.n_cams, rig.n_imgs, rig.n_keys)
        ps = np.concatenate([rig.intr.ravel(), rig.extr.ravel(), rig.poses.ravel()])

        # (1) sharded evaluation + gather (blocks moved to the host for gloo)
        local = sharding.make_engine_eval("template", det, counts, rig.points, rank=rank, world=world, device=device)

        def local_cpu(p, want_resid=True, want_jac=True):
            r, j = local(p, want_resid, want_jac)
            torch.cuda.synchronize()
            return (r.cpu() if r is not None else None), (j.cpu() if j is not None else None)

        # RCCL: the blocks stay on the GPUs and all_gather_into_tensor moves them over xGMI; gloo: through the host
        ev = sharding.ShardedEvaluator(det.shape[0], 21, local if rccl else local_cpu)
        r, j = ev.eval_gathered(ps)
        full = Engine("template", *counts, device=device)
        full.set_detections_table(det)
        full.set_template(rig.points)
        r0, j0 = full.eval(ps)
        assert np.array_equal(r.cpu().numpy(), r0) and np.array_equal(j.cpu().numpy(), j0)
        vec_reduce = sharding.allreduce_sum_fn(device=torch.device("cuda", device) if rccl else None)

        # (2) all-reduced matrix-free products on unpadded shards == single-process products
        per = sharding.shard_rows(det.shape[0], world)
        mine = det[rank * per:(rank + 1) * per]
        eng = Engine("template", *counts, device=device)
        eng.set_detections_table(mine)
        eng.set_template(rig.points)
        mask = np.ones(ps.shape[0], bool)
        mask[15 * rig.n_cams: 15 * rig.n_cams + 6] = False
        op = JacobianOperator(eng, mask, reduce_fn=vec_reduce)
        ref = JacobianOperator(full, mask)
        op.linearize(ps)
        ref.linearize(ps)
        v = np.random.default_rng(0).standard_normal(op.n_free)
        for a, b in ((op.jtjv(v), ref.jtjv(v)), (op.diag(), ref.diag()), (op.grad()[0], ref.grad()[0])):
            assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b))

        # (3) sharded device LM: every rank holds a handler over its shard with the GLOBAL layout
        names = [f"cam_{i}" for i in range(rig.n_cams)]

        def handler(rows):
            return handlers.TemplateBundleHandler(_Camset(rig.n_cams), _Target(rig.points),
                                                  TargetDetection(names, rows, max_ims=rig.n_imgs),
                                                  fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}},
                                                  options={"verbosity": 0}, counts=counts, device=device)

        h_shard, h_full = handler(mine), handler(det)
        bp = h_full.bundlePrimitive
        x0 = np.concatenate([rig.intr[bp.intr_unfixed].ravel(), rig.extr[bp.extr_unfixed].ravel(), rig.poses[bp.poses_unfixed].ravel()])
        res = lm_solve(h_shard, x0.copy(), max_iter=20, reduce_fn=vec_reduce, linear_solver="pcg")
        one = lm_solve(h_full, x0.copy(), max_iter=20, linear_solver="pcg")
        assert abs(res.cost - one.cost) <= 1e-5 * one.cost and res.cost < 0.01 * res.history[0], (res.cost, one.cost, res.history[0])
        gathered = [None] * world
        dist.all_gather_object(gathered, res.x)
        assert all(np.array_equal(gathered[0], g) for g in gathered)      # every rank walked the same path
        # the same with the block-reduced normal equations: ranks all-reduce [J^T J, J^T r, cost]
        # RCCL: the packed [J^T J, J^T r, cost] tensor is all-reduced in place on the device
        mat_reduce = sharding.allreduce_sum_tensor_fn() if rccl else sharding.allreduce_sum_fn()
        chol = lm_solve(h_shard, x0.copy(), max_iter=20, reduce_fn=mat_reduce, linear_solver="cholesky")
        assert abs(chol.cost - one.cost) <= 1e-5 * one.cost, (chol.cost, one.cost)
        dist.all_gather_object(gathered, chol.x)
        assert all(np.array_equal(gathered[0], g) for g in gathered)
        # ONE rank's one-launch dense solve gives up (1 us time limit on rank 1 only): the verdict travels with the all-reduced blocks,
        # so EVERY rank voids that trial, switches to the launch-per-column solve and repeats it — nobody adopts a garbage step and
        # nobody is left alone in a collective (the retry used to be decided per rank)
        eng_shard = h_shard.op_fun._engine_for(h_shard._flat_detections())
        if rank == 1:
            eng_shard.set_option("spd_timeout_us", 1)
        void = lm_solve(h_shard, x0.copy(), max_iter=20, reduce_fn=mat_reduce, linear_solver="cholesky")
        eng_shard.set_option("spd_timeout_us", 250000)
        ne_shard = next(iter(eng_shard.__dict__["_blocked_solvers"].values()))
        assert ne_shard.spd_algorithm == "launches", (rank, ne_shard.spd_algorithm)
        assert abs(void.cost - chol.cost) <= 1e-9 * chol.cost and (void.nit, void.nfev) == (chol.nit, chol.nfev), (void.cost, chol.cost, void.nfev, chol.nfev)
        dist.all_gather_object(gathered, void.x)
        assert all(np.array_equal(gathered[0], g) for g in gathered)

        # (4) self-calibration sharded: the global feature-visibility mask keeps the x layout identical
        vis = np.isin(np.arange(rig.n_keys), det[:, 2])

        def self_handler(rows):
            return handlers.SelfBundleHandler(_Camset(rig.n_cams), _Target(rig.points),
                                              TargetDetection(names, rows, max_ims=rig.n_imgs),
                                              fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}},
                                              options={"verbosity": 0}, counts=counts, visible_feature_mask=vis, device=device)

        s_shard, s_full = self_handler(mine), self_handler(det)
        assert np.array_equal(s_shard._jac_mask(), s_full._jac_mask())
        bs = s_full.bundlePrimitive
        xs = np.concatenate([rig.intr[bs.intr_unfixed].ravel(), rig.extr[bs.extr_unfixed].ravel(),
                             rig.poses[bs.poses_unfixed].ravel(), rig.points.ravel()[bs.bdpt_unfixed]])
        rs = lm_solve(s_shard, xs.copy(), max_iter=15, reduce_fn=vec_reduce, linear_solver="pcg")
        r1 = lm_solve(s_full, xs.copy(), max_iter=15, linear_solver="pcg")
        # default ("auto" = block-reduced normal equations + Schur step; the gauge-fixed point coordinates are permuted
        # into the leading group): exact steps end at least as low as the inexact CG steps.
        # round 5: a sharded loop runs in the engine's deterministic mode (device_solver._lm_solve_blocked switches it on): the normal
        # equations are summed in a fixed order (csrc/ba_reduce.hpp) and the K split of S -= V V' is subtracted in a fixed order, so
        # every rank computes the same bits from the all-reduced blocks and NO consensus step (one more collective per trial) is taken
        from pycamset_amd import device_solver as ds
        calls = []
        original = ds.BlockedNormalEquations._consensus_step
        ds.BlockedNormalEquations._consensus_step = lambda self, *a: calls.append(1) or original(self, *a)
        try:
            ra = lm_solve(s_shard, xs.copy(), max_iter=15, reduce_fn=mat_reduce)
            assert not calls, "deterministic mode takes no consensus step"
            assert ra.cost <= r1.cost * (1 + 1e-3), (ra.cost, r1.cost)
            # this system (192 leading x 192 trailing) makes schur_syrk_kernel split K (ksplit = 2)
            lay = s_shard.op_fun._engine_for(s_shard._flat_detections()).normal_layout()
            assert lay["n_trail"] > 128, lay
            dist.all_gather_object(gathered, (ra.x, ra.nit, ra.nfev, ra.status))
            assert all(np.array_equal(gathered[0][0], g[0]) and gathered[0][1:] == g[1:] for g in gathered)
            # where the mode is not available (the self chain beyond DET_SELF_CAM_LIMIT cameras keeps its atomics: partial sums meet in
            # arrival order) the loop is host-steered and the ranks adopt a consensus step per trial — they still walk ONE path
            limit, ds.DET_SELF_CAM_LIMIT = ds.DET_SELF_CAM_LIMIT, 0
            try:
                rc = lm_solve(s_shard, xs.copy(), max_iter=15, reduce_fn=mat_reduce)
            finally:
                ds.DET_SELF_CAM_LIMIT = limit
            assert calls, "the atomics build needs the consensus step"
            assert abs(rc.cost - ra.cost) <= 1e-6 * ra.cost, (rc.cost, ra.cost)
            dist.all_gather_object(gathered, (rc.x, rc.nit, rc.nfev, rc.status))
            assert all(np.array_equal(gathered[0][0], g[0]) and gathered[0][1:] == g[1:] for g in gathered)
        finally:
            ds.BlockedNormalEquations._consensus_step = original
        # self-calibration has a flat valley (gauge + point/pose trade-offs) and the J^T products sum with
        # f64 atomics in arrival order, so after 15 iterations the two runs agree in cost, not bit for bit
        assert abs(rs.cost - r1.cost) <= 1e-3 * r1.cost and rs.cost < 0.01 * rs.history[0], (rs.cost, r1.cost, rs.history[0])
        # (5) a GENERATED chain sharded (round 5): `projection + extrinsic3D + rigidTform3d + template_points` — two per-image transforms,
        # the last one the trailing entities of the blocked normal equations (csrc/ba_blockgram.hpp).  Every rank contracts the block rows
        # of ITS shard — in the ORDERED mode lm_solve switches on for a sharded loop —, the packed [A | B | C | g | cost] is all-reduced and
        # the exact step follows on every rank with the same bits: no consensus step (a chain whose blocks share a parameter group has no
        # ordered mode and would take one).
        from pycamset_amd import function_blocks as fb

        def gen_problem(rows):
            op_g = fb.optimisation_function([fb.projection(), fb.extrinsic3D(), fb.rigidTform3d(), fb.template_points()], counts=counts, device=device)
            assert op_g.chain == "generated"
            rng_g = np.random.default_rng(5)
            second = np.concatenate([rng_g.normal(0, 0.02, (rig.n_imgs, 3)), rng_g.normal(0, 0.002, (rig.n_imgs, 3))], axis=1)
            fix_ext = np.ones((rig.n_cams, 6), dtype=bool)
            fix_ext[0] = False
            start = [rig.intr, rig.extr.copy(), second, rig.poses]
            start[1][0] = rig.extr_true[0]
            # the middle transform is held (it is redundant with the pose behind it): the problem is the template chain's, through the generator
            return handlers.ChainProblem(op_g, rows, start, template=rig.points, unfixed=[None, fix_ext, np.zeros((rig.n_imgs, 6), dtype=bool), None])

        g_shard, g_full = gen_problem(mine), gen_problem(det)
        calls = []
        original = ds.BlockedNormalEquations._consensus_step
        ds.BlockedNormalEquations._consensus_step = lambda self, *a: calls.append(1) or original(self, *a)
        try:
            rg = lm_solve(g_shard, g_shard.x0.copy(), max_iter=20, reduce_fn=mat_reduce)
        finally:
            ds.BlockedNormalEquations._consensus_step = original
        rg1 = lm_solve(g_full, g_full.x0.copy(), max_iter=20)
        assert not calls and rg.n_jtjv == rg.nfev - 1, (len(calls), rg.n_jtjv, rg.nfev)    # exact steps, no consensus: ordered sums on every rank
        assert abs(rg.cost - rg1.cost) <= 1e-6 * rg1.cost and rg.cost < 0.01 * rg.history[0], (rg.cost, rg1.cost, rg.history[0])
        dist.all_gather_object(gathered, (rg.x, rg.nit, rg.nfev, rg.status))
        assert all(np.array_equal(gathered[0][0], g[0]) and gathered[0][1:] == g[1:] for g in gathered)
        Path(out_dir, f"ok{rank}").write_text("ok")
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), "gloo"), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one GPU per rank: this box has fewer than two")
def test_ranks_on_their_own_gpus_over_rccl(tmp_path):
    """The same assertions with backend nccl (RCCL over xGMI), one device per rank, every GPU of the box up to 8 ranks."""
    world = min(8, torch.cuda.device_count())
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), "nccl"), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


# ---- real shards with noise weights, a robust loss and a prior through lm_solve, one process per rank ------------------------------------
SPAWN_TIME_LIMIT = 300.0        # seconds: a rank left alone in a collective ends the test instead of hanging the suite


def _spawn(fn, args, world):
    import time
    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + SPAWN_TIME_LIMIT
    while not ctx.join(timeout=2.0):          # raises as soon as one rank has failed (and ends the others)
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail(f"the ranks did not finish within {SPAWN_TIME_LIMIT:.0f} s")


def _settings_worker(rank, world, port, out_dir, backend="gloo"):
    """Three ranks hold 60 %, 40 % and none of the ring-4 table (tests/sharded_sum_reference.py ``split(det, "empty")``), each with
    its own slice of a per-detection sigma; every setting is solved sharded and — on rank 0 — unsharded on the whole table."""
    import datetime
    sys.path.insert(0, str(REPO))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    rccl = backend == "nccl"
    device = rank if rccl else 0
    torch.cuda.set_device(device)
    limit = datetime.timedelta(seconds=120)
    if rccl:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device), timeout=limit)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=limit)
    try:
        from pycamset_amd import handlers, sharding
        from pycamset_amd.detections import TargetDetection
        from pycamset_amd.device_solver import lm_solve
        from tests import prior_reference as PR
        from tests import sharded_sum_reference as S

        assert world == 3
        vec_reduce = sharding.allreduce_sum_fn(device=torch.device("cuda", device) if rccl else None)
        mat_reduce = sharding.allreduce_sum_tensor_fn() if rccl else sharding.allreduce_sum_fn()
        gathered = [None] * world

        def same_on_every_rank(res):
            dist.all_gather_object(gathered, (res.x, res.nit, res.nfev, res.status))
            assert all(np.array_equal(gathered[0][0], g[0]) and gathered[0][1:] == g[1:] for g in gathered), [g[1:] for g in gathered]

        def from_rank0(value):
            box = [value]
            dist.broadcast_object_list(box, src=0)
            return box[0]

        for chain in ("template", "self"):
            for setting in ("weights", "weights+huber", "prior", "prior+weights+huber"):
                p = S.problem("ring4", chain, setting)
                rig, det, n = p.rig, p.det, p.det.shape[0]
                names = [f"cam_{i}" for i in range(rig.n_cams)]
                vis = np.isin(np.arange(rig.n_keys), det[:, 2])
                cls, extra = (handlers.TemplateBundleHandler, {}) if chain == "template" else (handlers.SelfBundleHandler, {"visible_feature_mask": vis})

                def handler(rows):     # the GLOBAL layout on every rank: counts, max_ims and, for self, the visibility mask
                    return cls(_Camset(rig.n_cams), _Target(rig.points), TargetDetection(names, rows, max_ims=rig.n_imgs),
                               fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0}, counts=p.counts, device=device, **extra)

                def solve(h, reduce_fn, sigma, **kw):
                    prior = {} if p.free_prior is None else dict(prior_mean=p.free_prior[0], prior_sigma=p.free_prior[1])
                    return lm_solve(h, p.x0.copy(), max_iter=200, reduce_fn=reduce_fn, loss=p.loss, f_scale=p.f_scale, sigma=sigma, **prior, **kw)

                def check_against(res, one, tol, what):
                    cost = from_rank0(None if one is None else one.cost)
                    assert abs(res.cost - cost) <= tol * cost, (what, rank, res.cost, cost)
                    if p.free_prior is not None:       # the prior is counted once, whatever the number of ranks
                        w = PR.weights_of(p.free_prior[1])
                        assert res.prior_cost > 0.0 and abs(res.prior_cost - PR.prior_half_sum(res.x, p.free_prior[0], w)) <= 1e-12 * res.prior_cost, (what, rank)
                    same_on_every_rank(res)

                what = f"{chain} {setting}"
                parts = p.parts("empty")
                mine = det[parts[rank]]
                assert [det[r].shape[0] for r in parts] == [(6 * n) // 10, n - (6 * n) // 10, 0]
                sig = None if p.sigma is None else {"detection": p.sigma["detection"][parts[rank]]}
                h_shard = handler(mine)
                h_full = handler(det) if rank == 0 else None
                assert np.array_equal(h_shard._jac_mask(), p.mask)
                res = solve(h_shard, mat_reduce, sig)
                one = solve(h_full, None, p.sigma) if rank == 0 else None
                check_against(res, one, 1e-9, what)
                if setting == "prior":     # matrix-free products: _PriorOperator wraps the REDUCED products, it is not reduced itself
                    cg = solve(h_shard, vec_reduce, None, linear_solver="pcg")
                    cg1 = solve(h_full, None, None, linear_solver="pcg") if rank == 0 else None
                    assert cg.n_jtjv > cg.nfev
                    check_against(cg, cg1, 1e-3, what + " pcg")
                if setting == "weights" and chain == "template":
                    # the split of sharding.shard_rows, the sigma through sharding.shard_sigma: the slices match
                    per = sharding.shard_rows(n, world)
                    rows = slice(rank * per, (rank + 1) * per)
                    part = sharding.shard_sigma(p.sigma, n, rank, world)
                    assert np.array_equal(part["detection"], p.sigma["detection"][rows]) and part["detection"].shape[0] == det[rows].shape[0]
                    bare = sharding.shard_sigma(p.sigma["detection"], n, rank, world)
                    assert np.array_equal(bare["detection"], part["detection"])
                    eq = solve(handler(det[rows]), mat_reduce, part)
                    check_against(eq, one, 1e-9, what + " shard_rows")
                torch.cuda.synchronize()
                eng = h_shard.op_fun._engine_for(h_shard._flat_detections())
                assert eng.n == mine.shape[0]
                assert eng.prior() is None and eng.weights() is None and eng.loss() == ("linear", 1.0), (what, rank)
        Path(out_dir, f"ok{rank}").write_text("ok")
    finally:
        dist.destroy_process_group()


def test_three_ranks_with_weights_loss_and_prior_on_one_gpu(tmp_path):
    """60 % / 40 % / empty shards of ring-4 over gloo, template and self: linear + sigma, huber + sigma, linear + prior (also through
    linear_solver="pcg"), huber + sigma + prior, each against the unsharded solve of the whole table: cost within 1e-9 relative (1e-3
    for pcg), the prior's half sum counted once, the same (x, nit, nfev, status) bits on every rank, the engines' settings restored."""
    world = 3
    _spawn(_settings_worker, (world, _free_port(), str(tmp_path), "gloo"), world)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


@pytest.mark.skipif(torch.cuda.device_count() < 3, reason="RCCL needs one GPU per rank: this box has fewer than three")
def test_three_ranks_with_weights_loss_and_prior_over_rccl(tmp_path):
    """The same worker with backend nccl (RCCL), one device per rank: the device-steered sharded loop under a real all-reduce."""
    world = 3
    _spawn(_settings_worker, (world, _free_port(), str(tmp_path), "nccl"), world)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))
