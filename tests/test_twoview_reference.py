"""The NumPy restatement of the two-view consensus (tests/twoview_reference.py) pinned on the CPU: it recovers true poses, its consensus
finds exactly the unmoved rows, its own rounding (float64 against extended precision) gives the bounds of tests/test_gpu_twoview.py, and
no parity input sits near a tie that rounding could flip."""
import numpy as np
import pytest

from tests import twoview_inputs as ti
from tests import twoview_reference as tv

# ceilings of the measured rounding (profiles/r26/README.md): d_T = 3.4e-13, d_s = 2.0e-9
D_T_CEILING, D_S_CEILING = 1e-12, 1e-8


@pytest.fixture(scope="module")
def measured():
    inputs = ti.parity_inputs()
    return inputs, tv.rounding(inputs)


def test_noise_free_pairs_recover_the_true_pose():
    """Three cameras, 40 keys, no noise, radius 5: every pair's (R, t / |t|) within CLEAN_POSE_BOUND (tests/twoview_inputs.py), every row an
    inlier in front of both cameras; and what 0.2 px of noise costs, printed (the sensitivity CLEAN_POSE_BOUND is derived from)."""
    for noise, bound in ((0.0, ti.CLEAN_POSE_BOUND), (0.2, None)):
        rig = ti.arc_rig(3, 40, noise, seed=11, radius=5.0)
        table = ti.table_of(rig, 3, 16)
        T, info, stats, inl, _ = tv.run_table(table, {"n_hypotheses": 16, "inlier_px": ti.INLIER_PX, "seed": 0, "min_points": 16})
        for p, (a, b) in enumerate(table["pairs"]):
            R, t = ti.relative_pose(rig, a, b)
            err = max(np.abs(T[p, :, :3] - R).max(), np.abs(T[p, :, 3] - t).max())
            print(f"noise {noise} pair ({a}, {b}): pose error {err:.2e}, info {info[p].tolist()}, parallax {stats[p, 2]:.3f}")
            if bound is not None:
                assert info[p].tolist()[:4] == [40, 40, 40, tv.OK] and err <= bound
                assert abs(np.linalg.det(T[p, :, :3]) - 1.0) < 1e-12 and abs(np.linalg.norm(T[p, :, 3]) - 1.0) < 1e-12


def test_consensus_returns_the_unmoved_rows():
    """30 % of a pair's rows replaced by uniformly random pixels: the inliers are exactly the unmoved rows, and the pose is that of the
    clean table."""
    rig, uv_a, uv_b, bad, moved = ti.outlier_pair()
    assert moved.sum() == 18
    opts = {"n_hypotheses": 64, "inlier_px": ti.INLIER_PX, "seed": 0, "min_points": 16}
    base = {"intr": rig["intr"], "pairs": np.array([[0, 1]], dtype=np.int32), "start": np.array([0, 60], dtype=np.int64), "uv_a": uv_a}
    T, info, _, inl, _ = tv.run_table({**base, "uv_b": bad}, opts)
    Tc, infoc, _, inlc, _ = tv.run_table({**base, "uv_b": uv_b}, opts)
    assert info[0, 3] == tv.OK and np.array_equal(inl, ~moved) and inlc.all()
    R, t = ti.relative_pose(rig, 0, 1)
    for pose in (T[0], Tc[0]):
        assert np.abs(pose[:, :3] - R).max() <= ti.CLEAN_POSE_BOUND and np.abs(pose[:, 3] - t).max() <= ti.CLEAN_POSE_BOUND


def test_statuses_of_pairs_that_cannot_be_estimated():
    few = ti.table_of(ti.one_pair(7), 2, 1)
    opts = {"n_hypotheses": 4, "inlier_px": ti.INLIER_PX, "seed": 0, "min_points": 8}
    T, info, stats, inl, _ = tv.run_table(few, opts)
    assert info[0].tolist() == [7, 0, 0, tv.TOO_FEW, -1] and np.all(np.isnan(T)) and np.all(np.isnan(stats)) and not inl.any()
    for rig in (ti.coplanar_pair(), ti.identical_cameras()):
        T, info, stats, inl, _ = tv.run_table(ti.table_of(rig, 2, 8), {**opts, "n_hypotheses": 16})
        ok = info[:, 3] == tv.OK
        print(info.tolist(), stats.tolist())
        assert np.all(np.isfinite(T[ok])) and np.all(np.isnan(T[~ok]))


def test_rounding_of_the_restatement(measured):
    """float64 against extended precision on the parity inputs: d_T over the entries of T against max(|entry|, 1), d_s relative over
    hypothesis scores and statistics.  Measured d_T = 3.4e-13 (pair-n8), d_s = 2.0e-9 (rig3-H16)."""
    _, rd = measured
    for name, (d_T, d_s, _) in rd.items():
        print(f"{name}: d_T {d_T:.2e}  d_s {d_s:.2e}")
    d_T, d_s = max(v[0] for v in rd.values()), max(v[1] for v in rd.values())
    print(f"d_T {d_T:.2e}  d_s {d_s:.2e}")
    assert 0.0 < d_T <= D_T_CEILING and 0.0 < d_s <= D_S_CEILING


def test_tie_condition_of_every_input(measured):
    """No Sampson distance at a winner lies within a relative 1e-6 of tau^2, and the winner's score is separated from the runner-up's by
    more than 1e-9 relative, or the two are the identical sample: rounding cannot flip a discrete output of a parity input."""
    from tests.pnp_consensus_reference import sample_positions

    inputs, rd = measured
    tau2 = ti.INLIER_PX ** 2
    for name, (table, opts) in inputs.items():
        for p, res in enumerate(rd[name][2][4]):
            if res["e2"] is not None:
                assert np.min(np.abs(res["e2"] - tau2)) > 1e-6 * tau2, (name, p)
            sc = res["scores"]
            if sc is None or sc.shape[0] < 2:
                continue
            order = np.argsort(sc, kind="stable")
            win, second = int(order[0]), int(order[1])
            n = int(table["start"][p + 1] - table["start"][p])
            same = np.array_equal(sample_positions(opts["seed"], p, n, win, tv.SAMPLE), sample_positions(opts["seed"], p, n, second, tv.SAMPLE))
            assert same or sc[second] - sc[win] > 1e-9 * sc[win], (name, p, sc[win], sc[second])


def test_table_building_takes_the_lowest_image_and_sorts_by_key():
    dct = np.array([[0, 1, 5, 10.0, 11.0], [0, 0, 5, 12.0, 13.0], [1, 0, 5, 20.0, 21.0], [1, 0, 3, 22.0, 23.0], [0, 2, 3, 14.0, 15.0],
                    [2, 0, 9, 1.0, 1.0]])
    pairs, start, keys, ua, ub = tv.correspondences(dct, 3, min_points=2)
    assert pairs.tolist() == [[0, 1]] and start.tolist() == [0, 2] and keys.tolist() == [3, 5]
    assert ua.tolist() == [[14.0, 15.0], [12.0, 13.0]] and ub.tolist() == [[22.0, 23.0], [20.0, 21.0]]
    from pycamset_amd import compiled_helpers as ch

    seen = ch.shared_keys(dct, 3)
    assert seen[0][0].tolist() == [3, 5] and seen[0][1].tolist() == [[14.0, 15.0], [12.0, 13.0]] and seen[2][0].tolist() == [9]


class _Tri:
    pass


def restated_entry_points():
    """The three device entry points of ``pose_seeding.seed_scene`` replaced by the restatements, with the device's signatures."""
    from pycamset_amd import compiled_helpers as ch
    from tests import pnp_reference as pref
    from tests import tri_refine_reference as tref

    def two_view(d, K, *, consensus, inlier_px, seed, min_points):
        pairs, start, keys, ua, ub = tv.correspondences(d, K.shape[0], min_points=min_points)
        T, info, stats, inl, _ = tv.estimate_pairs(ua, ub, start, pairs, K, n_hypotheses=consensus, inlier_px=inlier_px, seed=seed, min_points=min_points)
        return ch.TwoViewResult(pairs=pairs, T=T, n=info[:, 0], n_inliers=info[:, 1], n_front=info[:, 2], status=info[:, 3], hypothesis=info[:, 4],
                                score=stats[:, 0], rms=stats[:, 1], parallax=stats[:, 2], start=start, keys=keys, uv_a=ua, uv_b=ub, inliers=inl)

    def triangulate(rows, P, start, Km, D, **opts):
        intr = np.column_stack([Km[:, 0, 0], Km[:, 0, 2], Km[:, 1, 1], Km[:, 1, 2], D])
        out = _Tri()
        n = start.shape[0] - 1
        out.points, out.n_views, out.rms = np.full((n, 3), np.nan), np.zeros(n, dtype=np.int32), np.full(n, np.nan)
        for j in range(n):
            r = rows[start[j]:start[j + 1]]
            cams, uv = r[:, 0].astype(int).tolist(), r[:, 1:3]
            X, _, _ = tref.refine_point(tv.dlt_point(cams, uv, P, intr), cams, uv, P, Km, D)
            out.points[j], out.n_views[j], out.rms[j] = X, len(cams), tref.rms(X, cams, uv, P, Km, D)
        return out

    def view_poses(table, points, K, *, n_imgs, min_points, **opts):
        return pref.estimate_view_poses(table, points, K, n_cams=K.shape[0], n_imgs=n_imgs, min_points=min_points)

    return {"two_view_fn": two_view, "triangulate_fn": triangulate, "view_pose_fn": view_poses}


def test_scene_seed_of_the_restatement():
    """The chain rig (5 cameras, 60 keys, camera i shares keys only with i +- 1, i +- 2), noise-free: the restated pipeline places every
    camera in two rounds and, after a similarity alignment, agrees with truth within SCENE_GAP (measured: points 2.5e-12, camera centres
    5.6e-12 of the scene size, rotations 3.2e-12 rad).  ``pose_seeding.seed_scene`` on the same restatements takes the same decisions."""
    from pycamset_amd import pose_seeding

    rig = ti.chain_rig(0.0)
    ref = tv.seed_scene(rig["dct"], rig["intr"], 5, n_hypotheses=ti.SCENE_HYPOTHESES)
    gap = tv.scene_gap(ref["extr"], ref["points"], rig)
    print("restatement: first pair", ref["first_pair"], "rounds", ref["round_of_camera"].tolist(), "gap", gap)
    assert ref["placed"].all() and ref["round_of_camera"].max() == 2 and np.all(np.isfinite(ref["points"]))
    assert np.abs(ref["extr"][0]).max() < 1e-15 and ref["frame_cam"] == 0
    assert max(gap) <= ti.SCENE_GAP
    got = pose_seeding.seed_scene(rig["dct"], rig["intr"], 5, consensus=ti.SCENE_HYPOTHESES, **restated_entry_points())
    assert got.first_pair == ref["first_pair"] and np.array_equal(got.round_of_camera, ref["round_of_camera"]) and got.placed.all()
    assert np.allclose(got.extr, ref["extr"], rtol=0, atol=1e-9) and np.allclose(got.points, ref["points"], rtol=0, atol=1e-9)
    assert got.n_views.tolist() == [3] * 60 and np.all(got.rms < 1e-6)


def test_scene_seed_reports_what_it_could_not_place():
    """A camera that shares too few keys with the rest stays unplaced, ``ref_cam`` falls back to the first pair's camera a, and the
    arguments are validated before any work."""
    from pycamset_amd import pose_seeding

    rig = ti.chain_rig(0.0)
    d = rig["dct"]
    d = d[~((d[:, 0] == 4) & (d[:, 2] >= 30))]     # camera 4 keeps 10 keys: fewer than min_points
    got = pose_seeding.seed_scene(d, rig["intr"], 5, ref_cam=4, consensus=ti.SCENE_HYPOTHESES, **restated_entry_points())
    assert got.placed.tolist() == [True, True, True, True, False] and got.round_of_camera[4] == -1 and np.all(np.isnan(got.extr[4]))
    assert got.frame_cam == got.first_pair[0] and got.extr[got.frame_cam].tolist() == [0.0] * 6
    for kw in ({"ref_cam": 5}, {"baseline": 0.0}, {"consensus": 0}, {"inlier_px": -1.0}, {"min_points": 0}):
        with pytest.raises(ValueError):
            pose_seeding.seed_scene(d, rig["intr"], 5, **kw)
    with pytest.raises(ValueError):
        pose_seeding.seed_scene(d[:, :4], rig["intr"], 5)
