"""The C ABI of the PatchMatch depth (include/pcs_hip.h pcs_pm_*): the library exports every entry point, the binding knows them, and
every argument is refused on the host, without a GPU, with a message that names it."""
import ctypes
from pathlib import Path

import numpy as np

from pycamset_amd import _capi, patchmatch
from tests import fusion_inputs as fi

NAMES = ("pcs_pm_create", "pcs_pm_destroy", "pcs_pm_set_views", "pcs_pm_set_neighbours", "pcs_pm_init", "pcs_pm_iterate", "pcs_pm_finish", "pcs_pm_last_kernel_ms")


def _err():
    return _capi.lib().pcs_last_error().decode()


def test_the_pm_symbols_are_declared_bound_and_exported():
    lib = _capi.lib()
    header = (Path(__file__).resolve().parent.parent / "include" / "pcs_hip.h").read_text()
    for name in NAMES:
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
        assert f"{name}(" in header
    assert lib.pcs_version() >= 130
    assert (_capi.PM_NOT_STRICT, _capi.PM_NO_VIEW, _capi.PM_MAX_NEIGHBOURS) == (1, 2, 16) == (patchmatch.PM_NOT_STRICT, patchmatch.PM_NO_VIEW, patchmatch.PM_MAX_NEIGHBOURS)


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _capi.lib()
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    K, E = fi.ring_views(3, 8, 6, 8.0)
    K, P = np.ascontiguousarray(K), np.ascontiguousarray(E.reshape(3, 12))
    ARG = _capi.PCS_ERR_ARG
    assert lib.pcs_pm_create(None, 0) == ARG and lib.pcs_pm_destroy(None) == _capi.PCS_OK
    for args, word in (((0, 8, 6, dp(K), dp(P)), "n_views"), ((3, 0, 6, dp(K), dp(P)), "width"), ((3, 8, 6, None, dp(P)), "K"), ((3, 8, 6, dp(K), None), "P"),
                       ((3, 8, 6, dp(K), dp(P)), "NULL handle")):
        assert lib.pcs_pm_set_views(None, *args) == ARG and "pcs_pm_set_views" in _err() and word in _err(), (word, _err())
    for start, nbr, n, word in (([0, 1, 2, 3], [1, 0, 0], 0, "n 0"), (np.concatenate([[0], np.full(3, 17)]), np.arange(17) % 3, 3, "more than 16"),
                                ([0, 1, 2, 3], [1, 1, 0], 3, "own neighbour"), ([0, 1, 2, 3], [1, 0, 0], 3, "NULL handle")):
        assert lib.pcs_pm_set_neighbours(None, ip(start), ip(nbr), n) == ARG and "pcs_pm_set_neighbours" in _err() and word in _err(), (word, _err())
    wr, sm = np.array([[0.5, 1.0]]), np.full(3, 0.02)
    search = dict(d_images=64, pitch=8, wrange=dp(wr), n_w=1, slope_max=dp(sm), census_w=5, census_h=5, stride=1, truncate=6, seed=0)
    bad_search = ((dict(d_images=None), "d_images"), (dict(n_w=0), "n_w"), (dict(wrange=None), "wrange"), (dict(wrange=dp([[0.0, 1.0]])), "0 < w_lo < w_hi"),
                  (dict(wrange=dp([[1.0, 1.0]])), "w_lo < w_hi"), (dict(wrange=dp([[0.5, np.inf]])), "finite"), (dict(wrange=dp([[np.nan, 1.0]])), "finite"),
                  (dict(slope_max=None), "slope_max"), (dict(census_w=4), "census_w"), (dict(census_h=1), "census_h"), (dict(census_w=9, census_h=9), "bits"),
                  (dict(stride=0), "stride"), (dict(stride=5), "stride"), (dict(truncate=0), "truncate"), (dict(truncate=25), "truncate"))
    # pcs_pm_init: (search..., d_start_depth, start_dtype, start_planes, d_plane, d_cost, stream)
    rest = dict(d_start_depth=None, start_dtype=0, start_planes=0, d_plane=64, d_cost=64, stream=None)
    for change, word in bad_search + ((dict(d_plane=None), "d_plane"), (dict(d_cost=None), "d_cost"), (dict(d_start_depth=64, start_dtype=2), "start_dtype"),
                                      (dict(start_planes=2), "start_planes"), (dict(d_start_depth=64, start_dtype=1, start_planes=1), "exclude"), (dict(), "NULL handle")):
        a = dict(dict(search, **rest), **change)
        assert lib.pcs_pm_init(None, *a.values()) == ARG and "pcs_pm_init" in _err() and word in _err(), (word, _err())
    # pcs_pm_iterate: (first_iteration, n_iterations, search..., d_plane, d_cost, stream)
    rest = dict(d_plane=64, d_cost=64, stream=None)
    for first, n, change, word in [(0, 1, c, w) for c, w in bad_search] + [(-1, 1, {}, "first_iteration"), (1001, 0, {}, "first_iteration"), (0, -1, {}, "n_iterations"),
                                                                           (999, 2, {}, "n_iterations"), (0, 1, dict(d_plane=None), "d_plane"), (0, 1, {}, "NULL handle")]:
        a = dict(dict(search, **rest), **change)
        assert lib.pcs_pm_iterate(None, first, n, *a.values()) == ARG and "pcs_pm_iterate" in _err() and word in _err(), (word, _err())
    # pcs_pm_finish: (census_w, census_h, stride, truncate, d_plane, d_cost, d_depth, depth_dtype, d_normal, d_status, stream)
    ok = dict(census_w=5, census_h=5, stride=1, truncate=6, d_plane=64, d_cost=64, d_depth=64, depth_dtype=1, d_normal=None, d_status=None, stream=None)
    for change, word in ((dict(census_w=2), "census_w"), (dict(stride=9), "stride"), (dict(truncate=99), "truncate"), (dict(d_plane=None), "d_plane"), (dict(d_cost=None), "d_cost"),
                         (dict(d_depth=None), "d_depth"), (dict(depth_dtype=2), "depth_dtype"), (dict(), "NULL handle")):
        a = dict(ok, **change)
        assert lib.pcs_pm_finish(None, *a.values()) == ARG and "pcs_pm_finish" in _err() and word in _err(), (word, _err())
    f = ctypes.c_float()
    assert lib.pcs_pm_last_kernel_ms(None, ctypes.byref(f)) == ARG
    if lib.pcs_device_count() == 0:   # no device: no handle, and never a CPU fallback
        try:
            patchmatch.PatchMatcher(0)
        except _capi.PcsError as e:
            assert e.code == _capi.PCS_ERR_NODEVICE
        else:
            raise AssertionError("a handle without a device")
