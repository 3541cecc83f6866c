"""The sharded LM loops under a collective that really sums (the other device tests of a sharded loop use an identity).

1: several ranks' solver states in ONE process (``stepwise_ranks``): every rank builds the trial state of its own rows, the driver sums
   the states over the ranks between the two halves of a trial (pcs_lm_trial_build / pcs_lm_trial_finish), and every trial is held
   against the oracle of the whole table with the whole weight vector, the loss and the prior added once
   (tests/sharded_sum_reference.py), through ``check_trials`` of tests/test_gpu_lm_trials.py; all ranks must hold the same bits.
   Unequal shards, an empty shard, a shard of one camera; noise weights, robust losses, a prior; void votes that sum to 1 and 3.
2: the real loops (``lm_solve`` through ``_lm_loop_device`` and ``_lm_loop_blocked``) under a stand-in that multiplies by k = 2, 3 —
   k ranks holding the same shard — against the unsharded solve of the table repeated k times."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest

from tests import lm_reference as R
from tests import prior_reference as PR
from tests import sharded_sum_reference as S
from tests.test_gpu_lm_trials import _report, check_trials

pytestmark = pytest.mark.gpu
SPD_TIMEOUT_DEFAULT = 250000        # include/pcs_hip.h: option "spd_timeout_us"


# ================================================================================ 1: several ranks in one process, trial by trial

class Ranks:
    """One engine and one solver state per rank, all on device 0, for the problem ``p`` split into ``parts``; and what ``check_trials``
    asks of its fixture: the mask, the layout, the oracle of the WHOLE table."""

    def __init__(self, p, parts):
        import torch
        from pycamset_amd.device_solver import BlockedNormalEquations
        from pycamset_amd.engine import Engine
        self.p, self.parts, self.mask = p, parts, p.mask
        self.dev = torch.device("cuda", 0)
        self.engs, self.nes = [], []
        for rows in parts:
            # the global counts on every rank; an empty rank has the layout and no detections (function_blocks._engine_for, counts=)
            eng = Engine(p.chain, *p.counts, device=0)
            eng.set_detections_table(np.ascontiguousarray(p.det[rows]).reshape(-1, 5))
            if p.tm is not None:
                eng.set_template(p.tm)
            self.engs.append(eng)
            self.nes.append(BlockedNormalEquations(eng, p.mask))
        self.lay = self.engs[0].normal_layout()
        self.eng = SimpleNamespace(lm_fixed_trial_buffer=True)      # check_trials: an accepted trial is copied over state 0, nothing flips
        self.stream = torch.cuda.Stream(device=self.dev)            # ONE stream for every rank's kernels and the sums between them
        self.oracle, self.oracle_cost = p.oracle, p.oracle_cost

    @contextlib.contextmanager
    def settings(self):
        """Deterministic mode, the loss, each rank's own slice of the weights and the same prior on every rank; restored afterwards."""
        import torch
        p = self.p
        try:
            for eng, rows in zip(self.engs, self.parts):
                eng.set_option("deterministic", 1)
                eng.set_loss(p.loss, p.f_scale)
                eng.set_weights(inv_sigma=None if p.w is None else np.ascontiguousarray(p.w[rows]))
                if p.prior is not None:
                    eng.set_prior(p.prior[0], inv_sigma=p.prior[1])
            yield self
        finally:
            torch.cuda.synchronize()
            for eng in self.engs:
                eng.set_loss("linear", 1.0)
                eng.set_weights()
                eng.set_prior()
                eng.set_option("spd_timeout_us", SPD_TIMEOUT_DEFAULT)
                eng.set_option("deterministic", 0)

    def close(self):
        for eng in self.engs:
            eng.close()


def _sum_over_ranks(bufs):
    """What an all-reduce delivers: the sum in rank order, the same bits to every rank."""
    acc = bufs[0].clone()
    for b in bufs[1:]:
        acc += b
    for b in bufs:
        b.copy_(acc)


def stepwise_ranks(rk: Ranks, ctrl, lam0, max_trials=10, repeat_void=False):
    """Drive the ranks' solver states one trial at a time, the trial states summed over the ranks between pcs_lm_trial_build and
    pcs_lm_trial_finish.  -> per rank, per trial what ``stepwise`` of tests/test_gpu_lm_trials.py records, plus the summed trial state
    with its vote word (``pk_tri``).  ``repeat_void``: after a void trial every rank switches to the launch-per-column dense solve and
    the stop / accept flags are cleared, as ``_lm_loop_device`` does, and the drive goes on."""
    import torch
    from pycamset_amd._capi import LM_FIXED_TRIAL_BUFFER, LM_VOTES
    mode = LM_FIXED_TRIAL_BUFFER | LM_VOTES
    nes, engs, dev, p = rk.nes, rk.engs, rk.dev, rk.p
    npk = nes[0].n_packed
    sh = rk.stream.cuda_stream
    recs = [[] for _ in nes]
    torch.cuda.synchronize()
    with torch.cuda.device(dev), torch.cuda.stream(rk.stream):
        st = []
        for ne in nes:
            ps = [torch.from_numpy(p.ps0.copy()).to(dev), None]
            ps[1] = torch.empty_like(ps[0])
            st.append(dict(ps=ps, lam=torch.full((1,), float(lam0), dtype=torch.float64, device=dev),
                           ctrl=torch.from_numpy(np.array(ctrl, dtype=np.float64)).to(dev), flags=torch.zeros(4, dtype=torch.int32, device=dev),
                           stats=torch.zeros(12, dtype=torch.float64, device=dev)))
            for k in range(2):          # nothing of an earlier drive is left: whatever a build or an empty rank's zeroing does not write shows
                ne.packed[k][:npk].fill_(12345.0)
                ne.packed[k][npk] = 0.0
        # the start state: every rank's own rows (an empty rank: zeros, as BlockedNormalEquations.build), the sum, then the prior ONCE
        for ne, eng, q in zip(nes, engs, st):
            if eng.n == 0:
                ne.packed[0][:npk].zero_()
            else:
                eng.normal_blocks_device(q["ps"][0].data_ptr(), ne.packed[0].data_ptr(), sh)
        _sum_over_ranks([ne.packed[0] for ne in nes])
        for ne, eng, q in zip(nes, engs, st):
            eng.prior_add_device(q["ps"][0].data_ptr(), ne.packed[0].data_ptr(), sh)
        rk.stream.synchronize()
        for _ in range(max_trials):
            now = []
            for ne, q in zip(nes, st):
                cur = int(q["flags"][2].item())
                assert cur == 0, "a fixed trial buffer: state 0 stays current"
                now.append(dict(cur=cur, tri=1, sel=cur, ps_cur=q["ps"][0].cpu().numpy(), pk_cur=ne.packed[0][:npk].cpu().numpy(),
                                vote_cur=float(ne.packed[0][npk].item()), lam=float(q["lam"].item()), ctrl=q["ctrl"].cpu().numpy()))
            bufs = [ne.lm_buffers(q["ps"], q["lam"], q["ctrl"], q["flags"], q["stats"], mode=mode) for ne, q in zip(nes, st)]
            for eng, b in zip(engs, bufs):
                eng.lm_trial_build(b, sh)
            _sum_over_ranks([ne.packed[1] for ne in nes])                   # n_packed + 1 words: the vote word is summed with the state
            for eng, b in zip(engs, bufs):
                eng.lm_trial_finish(b, sh)
            rk.stream.synchronize()
            for ne, q, rec, out in zip(nes, st, now, recs):
                rec.update(delta=ne.delta.cpu().numpy(), dvec=ne.dvec.cpu().numpy(), gm=ne.gm.cpu().numpy(), ps_tri=q["ps"][1].cpu().numpy(),
                           c_new=float(ne.packed[1][npk - 1].item()), pk_tri=ne.packed[1].cpu().numpy(), stats=q["stats"].cpu().numpy(),
                           lam_after=float(q["lam"].item()), ctrl_after=q["ctrl"].cpu().numpy(), flags=q["flags"].cpu().numpy(),
                           ps_after=q["ps"][0].cpu().numpy(), pk_after=ne.packed[0].cpu().numpy(), status=int(ne.status.item()))
                out.append(rec)
            if recs[0][-1]["flags"][0]:
                if not (repeat_void and recs[0][-1]["stats"][8] == 9):
                    break
                for ne, q in zip(nes, st):
                    ne.spd_algorithm = "launches"
                    q["ctrl"][0] = 0.0
                    q["flags"][:2].zero_()
                rk.stream.synchronize()
    return recs


SAME_BITS = ("ps_cur", "pk_cur", "vote_cur", "lam", "ctrl", "delta", "dvec", "gm", "ps_tri", "c_new", "pk_tri", "stats", "lam_after", "ctrl_after",
             "flags", "ps_after", "pk_after")


def _bits(v):
    a = np.ascontiguousarray(v)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _b_masked(pk, lay, mask):
    """The packed state with B's rows and columns of fixed parameters at 0: what pcs_schur_prepare leaves of the state it reads (csrc/ba_schur.hpp)."""
    nl, nt = lay["n_lead"], lay["n_trail"]
    out = pk.copy()
    B = out[nl * nl: nl * nl + nl * nt].reshape(nl, nt)
    B[~mask[:nl], :] = 0.0
    B[:, ~mask[nl: nl + nt]] = 0.0
    return out


def assert_ranks_hold_the_same_bits(recs):
    """The promise ``_lm_solve_blocked`` relies on when it skips the consensus step: a condition, not a tolerance."""
    for r, other in enumerate(recs[1:], start=1):
        assert len(other) == len(recs[0]), (r, len(other), len(recs[0]))
        for k, (a, b) in enumerate(zip(recs[0], other)):
            for key in SAME_BITS:
                assert np.array_equal(_bits(np.asarray(a[key])), _bits(np.asarray(b[key]))), (f"rank {r} differs from rank 0", k, key)


# The start of a drive is `scale` x the rig's perturbation away from the truth, its first damping lam0; every drive must meet accepted AND
# rejected trials within its trials (checked on the first run, asserted below).
#   far:   the first, nearly undamped steps overshoot and are rejected (tests/test_gpu_lm_trials.py "ring8-template-far20").
#   damped / close / next to: starts whose drives were seen to reject a trial on the way.  The robust settings start near the solution,
#          as the robust fixtures of the suite do: from far away nearly every residual lies beyond f_scale, scipy's linearisation leaves
#          H = EPS J'J there, and the rejected trial points are so far out (costs of 1e40 and more) that their cost is not a
#          well-conditioned function of the string: nothing can be held to 1e-10 on it.  With a prior the drive keeps the default
#          tolerances and ends at ftol: driven on to rounding level, the detections' and the prior's gradients cancel and check_trials'
#          bound on g, which is relative to the gradient itself, no longer applies (6e-9 of a gradient of 43 was seen at such a state).
ACCEPT, REJECT = {"accept:fast", "accept:x1/3", "accept:x1", "accept:x2"}, {"reject:grow0", "reject:x4"}
FAR = dict(scale=20.0, lam0=1e-9, ctrl={})
DAMPED = dict(scale=5.0, lam0=1e-2, ctrl={})
CLOSE = dict(scale=0.3, lam0=1e-5, ctrl={})
NEXT_TO = dict(scale=0.05, lam0=1e-5, ctrl=dict(ftol=0.0, xtol=0.0, gtol=0.0))
STARTS = {"linear": FAR, "weights": FAR, "prior": DAMPED, "huber": NEXT_TO, "cauchy": NEXT_TO, "prior+weights+huber": CLOSE}
PART1_SETTINGS = tuple(STARTS)
# Every setting appears with the two-rank split and with the empty-rank split; the prior with weights and huber on both chains.
CASES = ([("ring4", "template", s, t) for s in ("two", "empty") for t in PART1_SETTINGS]
         + [("ring4", "template", "onecam", "linear"), ("ring4", "template", "onecam", "prior+weights+huber")]
         + [("ring4", "self", "two", "linear"), ("ring4", "self", "two", "huber"), ("ring4", "self", "two", "prior+weights+huber"),
            ("ring4", "self", "empty", "weights"), ("ring4", "self", "empty", "cauchy"), ("ring4", "self", "empty", "prior+weights+huber"),
            ("ring4", "self", "onecam", "prior"), ("ring8", "self", "empty", "prior")])


def _start(rig, setting):
    return FAR if rig == "ring8" else STARTS[setting]


def _case_id(c):
    return "-".join(c)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_every_trial_of_a_solve_summed_over_ranks(case, capsys):
    """Tolerances: those of ``check_trials``, unchanged (1e-10 on H, g and the costs against the oracle of the whole table, 1e-13
    backward error of the step, the decision exact away from the thresholds); the ranks agree bit for bit."""
    rig, chain, split, setting = case
    start = _start(rig, setting)
    p = S.problem(rig, chain, setting, scale=start["scale"])
    rk = Ranks(p, p.parts(split))
    try:
        if rig == "ring8":
            assert rk.lay["n_trail"] > 128, "the ordered K split of schur_syrk is part of the sharded trial"
        if split == "empty":
            assert rk.engs[-1].n == 0
        with rk.settings():
            recs = stepwise_ranks(rk, R.make_ctrl(max_iter=30, **start["ctrl"]), start["lam0"], max_trials=8 if rig == "ring8" else 14)
        assert_ranks_hold_the_same_bits(recs)
        assert all(rc["pk_tri"][-1] == 0.0 for rc in recs[0]), "nobody voted"
        labels, near = check_trials(rk, recs[0])
        _report(capsys, _case_id(case), labels, near)
        assert near == 0, (case, near)
        for need in (ACCEPT, REJECT):
            assert labels & need, (case, need, labels)
    finally:
        rk.close()


@pytest.mark.parametrize("givers", [(2,), (0, 1, 2)], ids=["one-empty-rank-votes", "all-three-vote"])
def test_void_votes_that_sum_over_ranks(givers):
    """Three ranks (the last one empty: its vote word sits behind the state its build zeroes); the ranks in ``givers`` run their
    one-launch dense solve with a 1 us time limit, the project's give-up path.  The summed vote word is 1 or 3 (the kernel reads
    ``votes > 0``): every rank voids that trial and leaves state, string and damping alone, and the repeated trial — every rank on
    the launch-per-column solve, stop and accept flags cleared as ``_lm_loop_device`` does — equals bit for bit the same trial of a
    drive that used that solve from the start."""
    p = S.problem("ring8", "template", "prior+weights+huber", scale=NEXT_TO["scale"])
    ctrl, lam0, n_trials = R.make_ctrl(max_iter=30, **NEXT_TO["ctrl"]), NEXT_TO["lam0"], 3
    rk = Ranks(p, p.parts("empty"))
    try:
        with rk.settings():
            for ne in rk.nes:
                ne.spd_algorithm = "launches"
            want = stepwise_ranks(rk, ctrl, lam0, max_trials=n_trials)
            for ne in rk.nes:
                ne.spd_algorithm = "auto"
            for r in givers:
                rk.engs[r].set_option("spd_timeout_us", 1)
            got = stepwise_ranks(rk, ctrl, lam0, max_trials=n_trials + 1, repeat_void=True)
            assert all(ne.spd_algorithm == "launches" for ne in rk.nes)
        assert_ranks_hold_the_same_bits(want)
        assert len(want[0]) == n_trials and len(got[0]) == n_trials + 1
        for r, rank_recs in enumerate(got):
            void = rank_recs[0]
            assert void["pk_tri"][-1] == float(len(givers)), (r, void["pk_tri"][-1])
            assert void["status"] == 0, "the decision cleared the status word"
            assert void["stats"][0] == -1.0 and void["stats"][8] == 9.0 and void["flags"][0] == 1 and void["flags"][1] == 0, (r, void["stats"], void["flags"])
            assert np.array_equal(_bits(void["ps_after"]), _bits(void["ps_cur"])), r
            # (the step's preparation masks B in place — fixed rows and columns become 0 —, as in every trial; nothing else of the state moves)
            assert np.array_equal(void["pk_after"][:-1], _b_masked(void["pk_cur"], rk.lay, rk.mask)) and void["pk_after"][-1] == void["vote_cur"], r
            assert void["lam_after"] == void["lam"] and void["flags"][2] == 0, r
            for i in (R.REJ, R.ACC):
                assert void["ctrl_after"][i] == void["ctrl"][i], (r, i)
            assert void["ctrl_after"][R.STOP] == 9.0
        # the void trial counted as a trial (ctrl[8], stats[9]); nothing else of the repeated drive differs from the reference drive
        for r, rank_recs in enumerate(got):
            for k, (a, b) in enumerate(zip(rank_recs[1:], want[r])):
                for key in SAME_BITS:
                    x, y = (np.array(v[key], dtype=None if key == "flags" else np.float64) for v in (a, b))
                    if key in ("ctrl", "ctrl_after"):
                        assert x[R.TRIALS] == y[R.TRIALS] + 1.0, (r, k, key)
                        x[R.TRIALS] = y[R.TRIALS]
                    if key == "stats":
                        assert x[9] == y[9] + 1.0, (r, k)
                        x[9] = y[9]
                    if key == "pk_cur":          # the void trial's preparation has masked B of the state already
                        x, y = _b_masked(x, rk.lay, rk.mask), _b_masked(y, rk.lay, rk.mask)
                    assert np.array_equal(_bits(x), _bits(y)), (r, k, key)
    finally:
        rk.close()


# ==================================================================================== 2: the real loops under a summing stand-in

def _times_in_stream(k, seen=None):
    """k ranks holding the same shard, stream-ordered: the device-steered loop."""
    def reduce_fn(t):
        t.mul_(float(k))
        if seen is not None:
            seen.append(t[-1:].clone())        # the summed vote word of this state, read after the solve
        return t

    reduce_fn.on_device = True
    return reduce_fn


def _times_on_host(k):
    """The same through the host: the host-steered loop."""
    return lambda a: float(k) * np.asarray(a)


def _handler_like(p, det):
    from pycamset_amd import handlers
    from pycamset_amd.detections import TargetDetection
    from tests.test_host_logic import DuckCamset, DuckTarget
    rig = p.rig
    names = [f"cam_{i}" for i in range(rig.n_cams)]
    cls = handlers.TemplateBundleHandler if p.chain == "template" else handlers.SelfBundleHandler
    return cls(DuckCamset(rig.n_cams), DuckTarget(rig.points), TargetDetection(names, det),
               fixed_params={"cam_0": {"ext": rig.extr_true[0].copy()}}, options={"verbosity": 0})


def _solve_kw(p, k=1):
    kw = dict(max_iter=60, loss=p.loss, f_scale=p.f_scale, prior_mean=p.free_prior[0], prior_sigma=p.free_prior[1])
    if p.sigma is not None:
        key, s = next(iter(p.sigma.items()))
        kw["sigma"] = {key: np.tile(s, k) if key == "detection" else s}
    return kw


def _tiled_reference(p, k):
    """The unsharded solve of the table repeated k times, with the sigma repeated too, in the engine's deterministic mode."""
    from pycamset_amd.device_solver import lm_solve
    h = _handler_like(p, np.tile(p.det, (k, 1)))
    eng = h.op_fun._engine_for(h._flat_detections())
    eng.set_option("deterministic", 1)
    try:
        return lm_solve(h, p.x0.copy(), **_solve_kw(p, k))
    finally:
        eng.set_option("deterministic", 0)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("setting", ["prior", "prior+huber"])
@pytest.mark.parametrize("chain", ["template", "self"])
def test_the_real_loops_under_a_stand_in_that_sums_k_equal_shards(chain, setting, k):
    """``reduce_fn = t.mul_(k)`` (device-steered loop: speculation, read-back ring, the prior inside pcs_lm_trial_finish) and
    ``lambda a: k * a`` (host-steered loop: BlockedNormalEquations.build) against the unsharded solve of the table repeated k
    times.  Same message, nit, nfev; cost within 1e-9 relative (the tolerance between loops of tests/test_gpu_prior.py); x within
    1e-7 max |x| on the template chain; prior_cost is the prior's half sum at the result, once.  Every bound is one the suite already
    uses; the solves were seen to agree far inside them (cost to 7.3e-15 relative, x to 1.1e-14 max |x| on all eight fixtures, both
    loops), so the spread of the reference itself under a reordered table never had to be consulted."""
    from pycamset_amd.device_solver import lm_solve
    p = S.problem("ring4", chain, setting)
    ref = _tiled_reference(p, k)
    assert ref.prior_cost > 0.0 and ref.nit >= 2
    w = PR.weights_of(p.free_prior[1])
    for name, fn in (("device-steered", _times_in_stream(k)), ("host-steered", _times_on_host(k))):
        res = lm_solve(p.h, p.x0.copy(), reduce_fn=fn, **_solve_kw(p))
        print(f"[{chain} {setting} k={k} {name}] cost {res.cost:.15e} reference {ref.cost:.15e} rel {abs(res.cost - ref.cost) / ref.cost:.2e} "
              f"nit {res.nit}/{ref.nit} nfev {res.nfev}/{ref.nfev} |dx| {np.max(np.abs(res.x - ref.x)) / np.max(np.abs(ref.x)):.2e}")
        assert (res.message, res.nit, res.nfev) == (ref.message, ref.nit, ref.nfev), (name, res.message, res.nit, res.nfev, ref.message, ref.nit, ref.nfev)
        assert abs(res.cost - ref.cost) <= 1e-9 * ref.cost, (name, res.cost, ref.cost)
        if chain == "template":
            assert np.max(np.abs(res.x - ref.x)) <= 1e-7 * np.max(np.abs(ref.x)), name
        assert abs(res.prior_cost - PR.prior_half_sum(res.x, p.free_prior[0], w)) <= 1e-12 * res.prior_cost, name
        # the prior's share of the cost is counted once, not k times: the rest is k times the detections' share
        assert abs((res.cost - res.prior_cost) - (ref.cost - ref.prior_cost)) <= 1e-9 * ref.cost, name
    eng = p.h.op_fun._engine_for(p.h._flat_detections())
    assert eng.prior() is None and eng.weights() is None and eng.loss() == ("linear", 1.0)


def test_void_votes_under_the_summing_stand_in():
    """k = 3 with a 1 us time limit on the one-launch dense solve: the first trial's vote sums to 3, the solve switches to the
    launch-per-column form and ends with the (nit, nfev) and the cost (1e-9) of the solve without the limit — the assertions of the
    two-process worker's step (3) in tests/test_gpu_sharded.py."""
    import torch
    from pycamset_amd.device_solver import lm_solve
    p = S.problem("ring8", "template", "prior")
    eng = p.h.op_fun._engine_for(p.h._flat_detections())
    plain = lm_solve(p.h, p.x0.copy(), reduce_fn=_times_in_stream(3), **_solve_kw(p))
    seen = []
    fn = _times_in_stream(3, seen)
    eng.set_option("spd_timeout_us", 1)
    try:
        void = lm_solve(p.h, p.x0.copy(), reduce_fn=fn, **_solve_kw(p))
    finally:
        eng.set_option("spd_timeout_us", SPD_TIMEOUT_DEFAULT)
    torch.cuda.synchronize()
    ne = next(iter(eng.__dict__["_blocked_solvers"].values()))
    assert ne.spd_algorithm == "launches", ne.spd_algorithm
    votes = [float(v.item()) for v in seen]
    assert votes[0] == 0.0 and votes[1] == 3.0, votes[:4]          # the start state carries no vote; the first trial's sums to 3
    trials = np.array(void.trials)
    assert trials[0, 0] == -1.0 and trials[0, 8] == 9.0 and np.all(trials[1:, 0] >= 0.0), trials[:, [0, 8]]
    assert (void.nit, void.nfev) == (plain.nit, plain.nfev), (void.nit, void.nfev, plain.nit, plain.nfev)
    assert abs(void.cost - plain.cost) <= 1e-9 * plain.cost, (void.cost, plain.cost)
