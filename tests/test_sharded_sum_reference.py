"""The reference side of tests/test_gpu_sharded_sum.py, checked without a GPU, so that the harness cannot agree with a bug by construction:
the ranks' own oracle systems sum to the system of the whole table for every loss the device tests use, the helper that adds the prior
adds it once (and the check notices when it is added once per rank), and the table repeated k times has k times the system — the
reference of the summing stand-in collective ``t.mul_(k)``."""
import numpy as np
import pytest

from tests import sharded_sum_reference as S
from tests import weights_reference as W

TOL = 1e-12      # of the scales weights_reference.check uses: sqrt(H_ii H_jj), max(|g|, sqrt(H_ii g'g)), |cost| — sums of the same terms in another order


@pytest.mark.parametrize("chain", ["template", "self"])
@pytest.mark.parametrize("setting", list(S.SETTINGS))
def test_the_shards_systems_sum_to_the_whole_tables(chain, setting):
    p = S.problem("ring4", chain, setting)
    ps = p.ps0
    H, g, c, _ = p.system(ps)
    for name in S.SPLITS:
        parts = p.parts(name)
        rows = np.concatenate([np.arange(p.det.shape[0])[r] for r in parts])
        assert np.array_equal(np.sort(rows), np.arange(p.det.shape[0])), name                 # a partition of the table
        if name == "empty":
            assert p.det[parts[-1]].shape[0] == 0
        if name == "onecam":
            assert np.unique(p.det[parts[1], 0]).shape[0] == 1
        Hs, gs, cs, _ = p.shard_sum(ps, parts)
        W.check(Hs, gs, cs, H, g, c, tol=TOL)        # no slack: a row's loss weight does not depend on the shard it is in
    if p.loss != "linear":
        f = W.rows_of(p.weights_of()) * S.orc.full_loss(chain, p.det, ps, p.tm).reshape(-1)
        assert np.sum(np.abs(f) > p.f_scale) > 10, "the loss is not linear on these residuals"
    assert abs(p.oracle_cost(ps) - c) <= TOL * c


@pytest.mark.parametrize("chain", ["template", "self"])
@pytest.mark.parametrize("setting", ["prior", "prior+weights+huber"])
def test_the_prior_is_added_once(chain, setting):
    p = S.problem("ring4", chain, setting)
    ps = p.ps0
    mean, w = p.prior
    assert np.all(w[~p.mask] == 0.0) and 0 < np.count_nonzero(w) < p.mask.sum()        # some entries finite, some inf, none on a fixed parameter
    H0, g0, c0, _ = p.detections_system(ps)
    H, g, c, _ = p.system(ps)
    d = np.where(w > 0.0, w * (ps - mean), 0.0)
    assert np.array_equal(H - H0, np.diag(np.diag(H - H0)))
    assert np.all(np.abs(np.diag(H - H0) - w * w) <= 4 * np.spacing(np.diag(H)))
    assert np.all(np.abs((g - g0) - w * d) <= 4 * np.spacing(np.maximum(np.abs(g), np.abs(g0))))
    assert abs((c - c0) - float(d @ d)) <= 4 * np.spacing(c) and float(d @ d) > 1e-6 * c0
    for name in S.SPLITS:
        parts = p.parts(name)
        W.check(*p.shard_sum(ps, parts)[:3], H, g, c, tol=TOL)
        # the prior in front of the sum (once per rank): the bounds the device tests apply (1e-10) see it on H, g or the cost
        with pytest.raises(AssertionError):
            W.check(*p.shard_sum(ps, parts, prior_per_rank=True)[:3], H, g, c, tol=1e-10)


@pytest.mark.parametrize("chain", ["template", "self"])
@pytest.mark.parametrize("k", [2, 3])
def test_the_tiled_table_has_k_times_the_system(chain, k):
    """What ``reduce_fn = t.mul_(k)`` stands for: k ranks holding the same shard sum to the table repeated k times (with the sigma
    repeated too); the prior is not part of the repetition."""
    for setting in ("prior", "prior+weights+huber"):
        p = S.problem("ring4", chain, setting)
        ps = p.ps0
        H1, g1, c1, _ = p.detections_system(ps)
        Hk, gk, ck, _ = W.weighted_system(chain, np.tile(p.det, (k, 1)), ps, p.tm, np.tile(p.weights_of(), k), p.loss, p.f_scale, counts=p.counts)
        W.check(Hk, gk, ck, k * H1, k * g1, k * c1, tol=TOL)
        H, g, c = p.add_prior(Hk, gk, ck, ps)
        Hw, gw, cw = p.add_prior(H1, g1, c1, ps)
        with pytest.raises(AssertionError):          # k times the augmented system counts the prior k times
            W.check(k * Hw, k * gw, k * cw, H, g, c, tol=1e-10)
