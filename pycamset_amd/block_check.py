"""``abstract_function_block.test_self``: a user block's ``compute_jac`` checked against finite differences of its ``compute_fun``,
on the GPU, on the device bodies the chains run (the reference's test_self, afb:750-775, checks the numba bodies on the host).

The block's two bodies — device strings, or Python bodies translated by block_translate.py — are compiled with
csrc/ba_blockcheck.hpp (chain_compiler.compile_blockcheck) and evaluated by ``pcs_blockcheck`` at every point: ``fun``, ``jac``
and a fourth-order central difference of ``fun`` per column.  For a Python-bodied block the Python bodies also run here with
NumPy at the same points and must agree with the device's ``fun`` / ``jac``: that checks the translation itself.
"""
from __future__ import annotations

from ctypes import POINTER, c_double

import numpy as np

from ._capi import check, lib

PYTHON_MATCH_RTOL = 1e-12      # device vs Python bodies, relative to the output row's scale


def _points(info, params, inp, n_points: int, seed: int):
    """(M, NP + NINROW) rows [params | inp]: the reference's all-ones point and ``n_points`` seeded points near it, or the caller's."""
    nrow_in = 3 if info.templated else info.nin
    if params is None and inp is None:
        rng = np.random.default_rng(seed)
        near = 1.0 + rng.uniform(-0.25, 0.25, (int(n_points), info.n_params + nrow_in))
        return np.ascontiguousarray(np.concatenate([np.ones((1, info.n_params + nrow_in)), near], axis=0))
    p = None if params is None else np.atleast_2d(np.asarray(params, dtype=np.float64))
    x = None if inp is None else np.atleast_2d(np.asarray(inp, dtype=np.float64))
    m = (p if p is not None else x).shape[0]
    if p is None:
        p = np.ones((m, info.n_params))
    if x is None:
        x = np.ones((m, nrow_in))
    if nrow_in == 0:
        x = np.zeros((m, 0))
    if p.shape != (m, info.n_params) or x.shape != (m, nrow_in):
        raise ValueError(f"block {info.name}: params must be (M, {info.n_params}) and inp (M, {nrow_in}); got {p.shape} and {x.shape}")
    return np.ascontiguousarray(np.concatenate([p, x], axis=1))


def _python_outputs(block, info, pts):
    from .block_translate import body_function

    f_fun, f_jac = body_function(block, "compute_fun"), body_function(block, "compute_jac")
    nc = info.n_params + info.nin
    fun = np.zeros((pts.shape[0], info.nout))
    jac = np.zeros((pts.shape[0], info.nout, nc))
    mem_len = max(1, int(getattr(block, "array_memory", 0) or 0))
    for i, row in enumerate(pts):
        p, x = row[: info.n_params].copy(), row[info.n_params:].copy()
        o = np.zeros(info.nout)
        f_fun(p, x, o, np.zeros(mem_len))
        fun[i] = o
        o = np.zeros(info.nout * nc)
        f_jac(p, x, o, np.zeros(mem_len))
        jac[i] = o.reshape(info.nout, nc)
    return fun, jac


def check_block(block, params=None, inp=None, *, n_points: int = 1024, rtol: float = 1e-6, atol: float = 1e-9, seed: int = 0, device: int = 0) -> dict:
    from .chain_compiler import BUILTIN_KINDS, compile_blockcheck, user_block_info

    if type(block).__name__ in BUILTIN_KINDS and not getattr(block, "device_fun", None):
        raise NotImplementedError(f"{type(block).__name__} is a shipped block: its Jacobian is covered by the golden tests, test_self checks user blocks")
    info = user_block_info(block)
    pts = _points(info, params, inp, n_points, seed)
    m, nc = pts.shape[0], info.n_params + info.nin
    fun = np.empty((m, info.nout))
    jac = np.empty((m, info.nout, nc))
    fd = np.empty((m, info.nout, nc))
    path = compile_blockcheck(info)
    dp = POINTER(c_double)
    check(lib().pcs_blockcheck(str(path).encode(), int(device), info.n_params, info.nin, info.nout, int(info.templated), pts.ctypes.data_as(dp), m,
                               fun.ctypes.data_as(dp), jac.ctypes.data_as(dp), fd.ctypes.data_as(dp)))
    name = info.name
    for what, arr in (("fun", fun), ("jac", jac), ("finite difference", fd)):
        bad = np.argwhere(~np.isfinite(arr))
        if bad.size:
            at = tuple(int(v) for v in bad[0])
            where = f"point {at[0]}, output row {at[1]}" + (f", column {at[2]}" if len(at) > 2 else "")
            raise AssertionError(f"user block {name}: non-finite {what} at {where} (the point is {pts[at[0]].tolist()})")
    rowscale = np.maximum(1.0, np.maximum(np.abs(jac).max(axis=2, initial=0.0), np.abs(fd).max(axis=2, initial=0.0)))[:, :, None]
    err = np.abs(jac - fd)
    ratio = err / (atol * rowscale + rtol * np.abs(fd))
    report = {"block": name, "n_points": m, "max_error": err.max(axis=(0, 1)), "worst_ratio": float(ratio.max()) if ratio.size else 0.0,
              "python_max_rel": None}
    if ratio.size and ratio.max() > 1.0:
        pt, o, c = (int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        raise AssertionError(f"user block {name}: compute_jac disagrees with finite differences of compute_fun at output row {o}, column {c} "
                             f"(point {pt}: {pts[pt].tolist()}): jac = {jac[pt, o, c]!r}, finite difference = {fd[pt, o, c]!r} "
                             f"(|diff| {err[pt, o, c]:.3e} > atol {atol:g} x row scale {rowscale[pt, o, 0]:.3g} + rtol {rtol:g} x |fd|)")
    if info.translated:
        hfun, hjac = _python_outputs(block, info, pts)
        rel = 0.0
        for what, dev, host in (("compute_fun", fun[:, :, None], hfun[:, :, None]), ("compute_jac", jac, hjac)):
            scale = np.maximum(1.0, np.abs(host).max(axis=2, initial=0.0))[:, :, None]
            d = np.abs(dev - host) / scale
            if not np.all(np.isfinite(host)) or d.max() > PYTHON_MATCH_RTOL:
                pt, o, c = (int(v) for v in np.unravel_index(int(np.nanargmax(np.where(np.isfinite(d), d, np.inf))), d.shape))
                raise AssertionError(f"user block {name}: the translated {what} disagrees with the Python body at output row {o}, column {c} "
                                     f"(point {pt}): device {dev[pt, o, c]!r}, Python {host[pt, o, c]!r}")
            rel = max(rel, float(d.max()))
        report["python_max_rel"] = rel
    return report
