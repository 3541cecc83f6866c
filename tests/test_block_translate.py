"""User blocks with Python bodies (pycamset_amd/block_translate.py), without a GPU: the three blocks of tests/golden/_user_blocks.py
re-declared with plain Python bodies lay out, index and compile like the reference's generator and the device twins; every construct
of the supported subset computes what Python computes (the translated body built for the host with g++ and called through ctypes);
every construct outside it is refused with its line."""
import ctypes
import inspect
import math
import os
import re
import struct
import subprocess
import tempfile
import zlib
from pathlib import Path

import numpy as np
import pytest

from pycamset_amd import block_translate as bt
from pycamset_amd import chain_compiler as cc
from pycamset_amd import function_blocks as fb
from tests import helpers as H
from tests import python_blocks as PB

REPO = Path(__file__).resolve().parent.parent
SCALE, OFFSET, COUNT = 1.5, -0.25, 3        # module globals a body may read (frozen at translation time)


def _readobj():
    return Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "llvm-readobj"


def _gfx950_elf(path, tmp: Path) -> Path:
    """The code object itself: hiprtc writes a plain ELF, `hipcc --genco` (the compiler fall-back) a clang offload bundle around it."""
    blob = Path(path).read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    if not blob.startswith(magic):
        return Path(path)
    pos, (n,) = len(magic), struct.unpack_from("<Q", blob, len(magic))
    pos += 8
    for _ in range(n):
        off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
        triple = blob[pos + 24: pos + 24 + tlen].decode()
        pos += 24 + tlen
        if "gfx950" in triple:
            out = tmp / "gfx950.elf"
            out.write_bytes(blob[off: off + size])
            return out
    raise AssertionError(f"{path}: no gfx950 code object in the bundle")


def kernel_meta(path):
    """{kernel name: (vgpr_count, private_segment_fixed_size)} from the code object's metadata note."""
    with tempfile.TemporaryDirectory(prefix="pcs_co_") as tmp:
        text = subprocess.run([str(_readobj()), "--notes", str(_gfx950_elf(path, Path(tmp)))], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", text)
    vgpr = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", text)]
    priv = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(names) == len(vgpr) == len(priv) and names
    return dict(zip(names, zip(vgpr, priv)))


@pytest.mark.parametrize("tag", ["user_cam_scale", "user_division", "user_board_flex"])
def test_python_blocks_layout_structure_and_compilation(golden_dir, tag):
    g = np.load(golden_dir / f"{tag}.npz")
    names = [str(n) for n in g["blocks"]]
    spec = cc.ChainSpec.from_blocks(PB.chain_of(names))
    users = spec.user_blocks
    assert len(users) == 1 and users[0].translated
    det = g["detections"]
    C, I, K = (int(det[:, j].max()) + 1 for j in range(3))
    lay = spec.layout(C, I, K)
    assert lay["n_params"] == g["param_str"].shape[0] and spec.P == g["block_param_inds"].shape[1]
    cols = cc.block_param_inds(spec, lay, det[:, :3].astype(np.int64))
    assert np.array_equal(cols, g["block_param_inds"])
    idx, ptr, _, _ = cc.csr_structure_of(cols, lay["n_params"], None)
    assert np.array_equal(idx, g["indices_all"]) and np.array_equal(ptr, g["indptr_all"])
    idx, ptr, _, _ = cc.csr_structure_of(cols, lay["n_params"], g["unfixed"])
    assert np.array_equal(idx, g["indices_masked"]) and np.array_equal(ptr, g["indptr_masked"])
    text = cc.emit_source(spec)
    assert f'#include "{bt.PYBODY_HEADER}"' in text and "translated from" in text
    meta = kernel_meta(cc.compile_chain(spec))
    evals = {k: v for k, v in meta.items() if k.startswith(("pcs_genchain_eval", "pcs_genchain_compact"))}
    assert len(evals) == 20
    assert all(priv == 0 for _, priv in evals.values()), evals
    # the hand-translated device twin of tests/helpers.py compiles to the same register budget
    twin = kernel_meta(cc.compile_chain(cc.ChainSpec.from_blocks(PB.chain_of(names, H.user_blocks(fb)))))
    for k, (vgpr, _) in evals.items():
        assert abs(vgpr - twin[k][0]) <= 8, (k, vgpr, twin[k])


@pytest.mark.parametrize("name", ["cam_scale", "division_projection", "board_flex"])
def test_block_check_unit_compiles_without_scratch(name):
    info = cc.user_block_info(PB.python_blocks()[name]())
    assert info.translated and info.templated == (name == "board_flex")
    meta = kernel_meta(cc.compile_blockcheck(info))
    assert meta["pcs_blockcheck"][1] == 0


def test_device_strings_take_precedence_and_the_abc_has_no_bodies():
    twin = H.user_blocks(fb)["division_projection"]

    class both(twin):                    # device strings AND Python bodies: the strings win
        compute_fun = PB.division_projection.compute_fun
        compute_jac = PB.division_projection.compute_jac

    spec = cc.ChainSpec.from_blocks([both(), fb.extrinsic3D(), fb.template_points()])
    assert not spec.user_blocks[0].translated and spec.user_blocks[0].device_fun == twin.device_fun
    assert not cc.user_block_info(both()).translated
    assert not hasattr(fb.abstract_function_block, "compute_fun") and not hasattr(fb.abstract_function_block, "compute_jac")

    class neither(fb.abstract_function_block):
        num_inp, num_out = 3, 3
        params = fb.param_type(fb.key_type.PER_CAM, 1)

    with pytest.raises(NotImplementedError):
        cc.ChainSpec.from_blocks([fb.projection(), neither(), fb.extrinsic3D(), fb.template_points()])
    with pytest.raises(NotImplementedError):
        fb.projection().test_self()      # shipped blocks: the goldens cover them
    with pytest.raises(NotImplementedError):
        neither().test_self()


def test_numba_style_wrappers_are_unwrapped():
    class dispatcher:                    # what numba's @njit leaves: the Python function as .py_func
        def __init__(self, f):
            self.py_func = f

    class wrapped(fb.abstract_function_block):
        num_inp, num_out = 3, 2
        params = fb.param_type(fb.key_type.PER_CAM, 5)
        compute_fun = staticmethod(dispatcher(PB.division_projection.compute_fun))
        compute_jac = dispatcher(PB.division_projection.compute_jac)

    f1, j1 = bt.translate_block(wrapped())
    f2, j2 = bt.translate_block(PB.division_projection())
    strip = lambda s: "\n".join(s.splitlines()[1:])   # noqa: E731 (the first line names the block)
    assert strip(f1) == strip(f2) and strip(j1) == strip(j2)


# ---- differential check: the translated body on the host (g++) against the Python body -------------------------------------------------


def f_intdiv(params, inp, output, memory):
    a = int(params[0] * 10) - 5
    b = int(params[1] * 7) - 3
    if b == 0:
        b = 2
    output[0] = a // b
    output[1] = a % b
    output[2] = params[0] // (params[1] + 2.25) + params[0] // (params[1] - 2.25)
    output[3] = params[0] % (params[1] - 2.25) + params[0] % (params[1] + 2.25)
    output[4] = -7 // 2 + (-7) % 3 + 7 % -3


def f_pow(params, inp, output, memory):
    x = params[0]
    output[0] = x ** -2
    output[1] = x ** -1
    output[2] = x ** 0
    output[3] = x ** 1
    output[4] = x ** 2
    output[5] = x ** 3
    output[6] = x ** 4
    output[7] = abs(x) ** 0.5 + abs(x) ** params[1]
    n = COUNT
    output[8] = n ** 2 + 2 ** -2


def f_logic(params, inp, output, memory):
    a, b, c = params[0], params[1], params[2]
    if a < b < c:
        output[0] = 1.0
    elif a >= b > c or not (a != b):
        output[0] = 2
    else:
        output[0] = -1
    output[1] = a if 0 <= a <= 1 else b
    output[2] = min(a, b) + max(b, c) + min(1, 2) * max(3, COUNT)
    output[3] = 1.0 if (a > 0 and b > 0) or c > 1.5 else 0.0
    output[4] = float(a == b) + float(not a < 0)


def f_loops(params, inp, output, memory):
    output[:] = 0
    s = 0.0
    for i in range(4):
        s += params[i] * i
    output[0] = s
    n = int(abs(params[0]) * 3) + 1
    t = 0
    for j in range(1, n):
        t += j
    output[1] = t
    for k in range(6, -1, -2):
        output[2] += k * params[1]
    acc = 0.0
    m = 0
    for m in range(0, n + 3, 2):
        if m == 4:
            continue
        acc += m
        if acc > 8:
            break
    output[3] = acc
    output[4] = m
    for q in range(n, 0, -1 if params[2] > 0 else -2):
        output[5] += q


def f_math(params, inp, output, memory):
    x, y = params[0], params[1]
    ax = abs(x) + 0.1
    output[0] = math.sqrt(ax) + np.exp(y) - math.log(ax) + np.log1p(ax) + math.expm1(y)
    output[1] = math.sin(x) * np.cos(y) + math.tan(x * 0.3) + np.sinh(y) - math.cosh(x) + np.tanh(x)
    output[2] = np.arcsin(x / 3) + math.acos(y / 3) + np.arctan(x) + math.atan2(y, x) + np.arctan2(x, y) + math.asin(y / 4)
    output[3] = math.hypot(x, y) + np.hypot(y, 2.0)
    output[4] = math.floor(x) + np.ceil(y) + math.fabs(x) + np.abs(y) + math.copysign(2.0, y) + np.floor(x * 3)
    output[5] = float(int(x * 3)) + np.float64(2) / 3
    output[6] = math.pi * x + np.pi + math.e
    output[7] = SCALE * x + OFFSET


def f_views(params, inp, output, memory):
    k = params[2:]
    a, b = params[0], params[1]
    a, b = b, a
    x, y, z = inp
    memory[0] = a * x
    memory[1] = memory[0] + b * y
    o = output[1:]
    o[0] = memory[1] + k[0] * z + k[-1]
    output[0] = -a
    p, q = inp[1:]
    o[1] = p - q
    output[3] = memory[2]
    output[4:] = 0.5
    output[-1] += params[-1]


def f_types(params, inp, output, memory):
    i = 3
    j = i * 2 + COUNT
    output[0] = j / 4
    h = 7 // 2
    d = 2
    d = d * 0.5
    output[1] = 1 / 2 + h + d
    e = 1
    e += params[0]
    output[2] = e
    output[3] = int(params[1] * 4) * 2 - 1
    """a string in the middle of a body is a comment"""
    output[4] = True + (i > 2)


def f_return(params, inp, output, memory):
    output[0] = 1.0
    if params[0] > 0:
        output[1] = 2.0
        return
    pass
    output[1] = 3.0
    return None


# name -> (function, n_params, num_inp, num_out, array_memory, rtol)
DIFFERENTIAL = {
    "intdiv": (f_intdiv, 2, 0, 5, 0, 0.0),
    "pow": (f_pow, 2, 0, 9, 0, 4e-16),
    "logic": (f_logic, 3, 0, 5, 0, 0.0),
    "loops": (f_loops, 4, 0, 6, 0, 0.0),
    "math": (f_math, 2, 0, 8, 0, 1e-14),
    "views": (f_views, 4, 3, 7, 3, 0.0),
    "types": (f_types, 2, 0, 5, 0, 0.0),
    "return": (f_return, 1, 0, 2, 0, 0.0),
}


def _block_for(name, fn, npar, nin, nout, mem):
    return type(name, (fb.abstract_function_block,), {"num_inp": nin, "num_out": nout, "array_memory": mem,
                                                       "params": fb.param_type(fb.key_type.PER_CAM, npar),
                                                       "compute_fun": staticmethod(fn), "compute_jac": staticmethod(fn)})


@pytest.fixture(scope="module")
def host_library():
    """Every translated body of the table (fun) and of the three blocks (fun and jac) as an extern "C" host function, one g++ build."""
    units, entries = [f'#include "{bt.PYBODY_HEADER}"', "#include <cmath>"], {}
    cases = {k: _block_for(f"t_{k}", *v[:5])() for k, v in DIFFERENTIAL.items()}
    for k, blk in cases.items():
        entries[(k, "compute_fun")] = blk
    for k, klass in PB.python_blocks().items():
        for which in ("compute_fun", "compute_jac"):
            entries[(k, which)] = klass()
    names = {}
    for i, ((k, which), blk) in enumerate(entries.items()):
        body = bt.translate_body(blk, which)
        fname = f"body_{i}"
        names[(k, which)] = fname
        units += [f"static void {fname}_one(const double *params, const double *inp, double *out) {{", body, "}",
                  f'extern "C" void {fname}(const double *P, int np, const double *X, int nin, double *O, int nout, int m) {{',
                  f"    for (int r = 0; r < m; ++r) {fname}_one(P + (long)r * np, X + (long)r * nin, O + (long)r * nout);", "}"]
    tmp = Path(tempfile.mkdtemp(prefix="pcs_bt_"))
    src, lib = tmp / "bodies.cpp", tmp / "bodies.so"
    src.write_text("\n".join(units) + "\n")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                    f"-I{REPO / 'pycamset_amd' / 'csrc'}", str(src), "-o", str(lib)], check=True, capture_output=True, text=True)
    return ctypes.CDLL(str(lib)), names, cases


def _run_host(lib, fname, P, X, nout):
    m = P.shape[0]
    out = np.zeros((m, nout))
    dp = ctypes.POINTER(ctypes.c_double)
    Xc = np.ascontiguousarray(X if X.size else np.zeros((m, 1)))
    getattr(lib, fname)(np.ascontiguousarray(P).ctypes.data_as(dp), P.shape[1], Xc.ctypes.data_as(dp), X.shape[1], out.ctypes.data_as(dp), nout, m)
    return out


def _run_python(fn, P, X, nout, mem):
    out = np.zeros((P.shape[0], nout))
    with np.errstate(all="ignore"):          # x ** -1 at x = 0: inf on both sides
        for r in range(P.shape[0]):
            o = np.zeros(nout)
            fn(P[r].copy(), X[r].copy(), o, np.zeros(max(1, mem)))
            out[r] = o
    return out


def _compare(got, want, rtol):
    same = (np.isnan(got) & np.isnan(want)) | (got == want)      # equal infinities and NaN in the same places count as agreement
    with np.errstate(invalid="ignore"):
        diff = np.where(same, 0.0, np.abs(got - want))
    assert np.all(np.isfinite(diff)), np.argwhere(~np.isfinite(diff))[:3]
    bad = diff > rtol * np.maximum(1.0, np.abs(want))
    assert not bad.any(), [(int(r), int(c), got[r, c], want[r, c]) for r, c in np.argwhere(bad)[:5]]


@pytest.mark.parametrize("case", sorted(DIFFERENTIAL))
def test_translated_constructs_compute_what_python_computes(host_library, case):
    lib, names, cases = host_library
    fn, npar, nin, nout, mem, rtol = DIFFERENTIAL[case]
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    P = rng.uniform(-2.0, 2.0, (1000, npar))
    P[:50] = np.round(P[:50] * 2) / 2          # exact halves and integers: ties of //, %, comparisons and floor
    X = rng.uniform(-2.0, 2.0, (1000, nin))
    _compare(_run_host(lib, names[(case, "compute_fun")], P, X, nout), _run_python(fn, P, X, nout, mem), rtol)


@pytest.mark.parametrize("name", ["cam_scale", "division_projection", "board_flex"])
def test_translated_user_blocks_compute_what_python_computes(host_library, name):
    lib, names, _ = host_library
    klass = PB.python_blocks()[name]
    npar, nin = klass.params.n_params, 3
    rng = np.random.default_rng(7)
    P = rng.uniform(0.5, 1.5, (1000, npar))
    X = rng.uniform(0.5, 1.5, (1000, nin))
    for which, nout in (("compute_fun", klass.num_out), ("compute_jac", klass.num_out * (npar + klass.num_inp))):
        fn = bt.body_function(klass(), which)
        _compare(_run_host(lib, names[(name, which)], P, X, nout), _run_python(fn, P, X, nout, 0), 0.0)


# ---- what the translator refuses ----------------------------------------------------------------------------------------------------------


def n_htform_prealloc(a, b):
    return a


def r_call(params, inp, output, memory):
    output[0] = params[0]
    n_htform_prealloc(params, output)  # BAD


def r_while(params, inp, output, memory):
    i = 0
    while i < 2:  # BAD
        i += 1


def r_list(params, inp, output, memory):
    a = [params[0], 1.0]  # BAD
    output[0] = a[0]


def r_dict(params, inp, output, memory):
    output[0] = {"a": 1}["a"]  # BAD


def r_comprehension(params, inp, output, memory):
    output[0] = sum([p for p in params])  # BAD


def r_np_empty(params, inp, output, memory):
    tmp = np.empty(3)  # BAD
    output[0] = tmp[0]


def r_np_zeros(params, inp, output, memory):
    output[0] = np.zeros(3)[0]  # BAD


def r_attribute_store(params, inp, output, memory):
    output.flags = 1  # BAD


def r_len(params, inp, output, memory):
    output[0] = len(params)  # BAD


def r_write_params(params, inp, output, memory):
    params[0] = 1.0  # BAD


def r_write_inp_view(params, inp, output, memory):
    v = inp[1:]
    v[0] = 2.0  # BAD


def r_index_out_of_range(params, inp, output, memory):
    output[0] = params[0]
    output[2] = 1.0  # BAD


def r_params_out_of_range(params, inp, output, memory):
    output[0] = params[3]  # BAD


def r_memory_out_of_range(params, inp, output, memory):
    memory[1] = 1.0  # BAD


def r_float_index(params, inp, output, memory):
    output[0] = params[params[0]]  # BAD


def r_unknown_name(params, inp, output, memory):
    output[0] = undefined_thing * 2  # BAD  # noqa: F821


REJECTED = [r_call, r_while, r_list, r_dict, r_comprehension, r_np_empty, r_np_zeros, r_attribute_store, r_len, r_write_params,
            r_write_inp_view, r_index_out_of_range, r_params_out_of_range, r_memory_out_of_range, r_float_index, r_unknown_name]


@pytest.mark.parametrize("fn", REJECTED, ids=[f.__name__ for f in REJECTED])
def test_unsupported_constructs_are_refused_with_their_line(fn):
    blk = _block_for("rejected_block", fn, 3, 3, 2, 0)()
    lines, start = inspect.getsourcelines(fn)
    line = start + next(i for i, text in enumerate(lines) if "# BAD" in text)
    with pytest.raises(NotImplementedError) as e:
        bt.translate_body(blk, "compute_fun")
    msg = str(e.value)
    assert f"test_block_translate.py:{line}" in msg, msg
    assert "rejected_block.compute_fun" in msg
    # through the chain compiler, too: a block whose bodies cannot be translated never reaches a chain
    with pytest.raises(NotImplementedError):
        cc.ChainSpec.from_blocks([blk, fb.extrinsic3D(), fb.template_points()])
