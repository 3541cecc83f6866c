"""Python-bodied user blocks -> the device bodies of a generated chain.

The reference's extension point is a subclass of ``abstract_function_block`` whose ``compute_fun`` / ``compute_jac`` are
(numba) Python functions; its code generator copies their source into the module it writes (afb:246-267, afb:424-463).
This module does the counterpart for the GPU: it reads a body with ``inspect.getsource``, parses it with ``ast`` and writes
the C++ statements that ``chain_compiler.emit_source`` pastes into ``void fun(const double *params, const double *inp,
double *out)`` / ``void jac(...)``, exactly where a ``device_function_block``'s hand-written strings go.  The rest of the
generator does not know the difference.

The accepted language is the subset numba-style block bodies use: scalar locals (``int`` or ``double``, inferred), tuple
assignment, arithmetic with Python's semantics (true ``/``, floor ``//`` and ``%``, ``**``), comparisons, ``and``/``or``/
``not``, ``if``, conditional expressions, ``for ... in range(...)``, subscripts and slice views of the four arrays, scalar
slice stores, and the scalar functions of ``math`` / ``np`` listed in ``_FUNCS``.  Anything else raises
``NotImplementedError`` naming the block, the body, the file and line and the offending source text: there is no
interpreter and no fallback.  Arguments are mapped by position (``params, inp, output, memory``) whatever their names;
``memory`` becomes a zero-initialised local array of ``max(1, array_memory)`` doubles.  Numeric module globals are frozen
at translation time.
"""
from __future__ import annotations

import ast
import inspect
import math
import os
import textwrap

INT, DBL, BOOL = "int", "double", "bool"
_ARRAYS = ("params", "inp", "out", "mem")          # C names of the four positional arguments
_READ_ONLY = ("params", "inp")
_MODULES = ("math", "np", "numpy")
# name -> (C function, arity, result type or None = double)
_FUNCS = {
    "sqrt": ("sqrt", 1), "exp": ("exp", 1), "log": ("log", 1), "log1p": ("log1p", 1), "expm1": ("expm1", 1),
    "sin": ("sin", 1), "cos": ("cos", 1), "tan": ("tan", 1), "sinh": ("sinh", 1), "cosh": ("cosh", 1), "tanh": ("tanh", 1),
    "asin": ("asin", 1), "acos": ("acos", 1), "atan": ("atan", 1), "arcsin": ("asin", 1), "arccos": ("acos", 1), "arctan": ("atan", 1),
    "atan2": ("atan2", 2), "arctan2": ("atan2", 2), "hypot": ("hypot", 2), "copysign": ("copysign", 2),
    "floor": ("floor", 1), "ceil": ("ceil", 1), "fabs": ("fabs", 1), "abs": ("fabs", 1), "absolute": ("fabs", 1),
}
_CONSTS = {"pi": math.pi, "e": math.e}
_CMP = {ast.Lt: "<", ast.LtE: "<=", ast.Gt: ">", ast.GtE: ">=", ast.Eq: "==", ast.NotEq: "!="}
_ARITH = {ast.Add: "+", ast.Sub: "-", ast.Mult: "*"}
MAX_SQUARING_EXPONENT = 16

PYBODY_HEADER = "ba_pybody.hpp"     # Python's floor division, modulo, min and max (csrc/ba_pybody.hpp), included by a unit with translated bodies

def _unwrap(fn):
    """The Python function behind a staticmethod / a numba dispatcher (``.py_func``) / a plain function."""
    for _ in range(4):
        if isinstance(fn, (staticmethod, classmethod)):
            fn = fn.__func__
        elif hasattr(fn, "py_func"):
            fn = fn.py_func
        else:
            break
    return fn


def body_function(block, which: str):
    """``compute_fun`` / ``compute_jac`` of a block's class as a plain Python function, or None."""
    for klass in type(block).__mro__:
        if which in klass.__dict__:
            fn = _unwrap(klass.__dict__[which])
            return fn if inspect.isfunction(fn) else None
    return None


def has_python_bodies(block) -> bool:
    return body_function(block, "compute_fun") is not None and body_function(block, "compute_jac") is not None


class _Array:
    """An array argument or a slice view of one: C expression of its base pointer, offset, known length, writability."""

    def __init__(self, cname: str, base: str, length: int, offset: int = 0):
        self.cname, self.base, self.length, self.offset = cname, base, length, offset

    @property
    def writable(self) -> bool:
        return self.base not in _READ_ONLY


def _lit(v, as_double: bool) -> str:
    if isinstance(v, bool):
        v = int(v)
    if isinstance(v, int) and not as_double:
        if not -(2 ** 31) <= v < 2 ** 31:
            raise ValueError(f"integer constant {v} does not fit an int")
        return str(v)
    v = float(v)
    if math.isnan(v):
        return "__builtin_nan(\"\")"
    if math.isinf(v):
        return "__builtin_huge_val()" if v > 0 else "(-__builtin_huge_val())"
    r = repr(v)
    return r if ("e" in r or "." in r) else r + ".0"


class _Translator:
    def __init__(self, block, which: str, fn, lengths: dict):
        self.block, self.which, self.fn = block, which, fn
        self.bname = type(block).__name__
        lines, self.first_line = inspect.getsourcelines(fn)
        self.file = inspect.getsourcefile(fn) or "<unknown>"
        self.src = textwrap.dedent("".join(lines))
        tree = ast.parse(self.src)
        fdefs = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
        if len(fdefs) != 1:
            raise self.err(tree, "the body must be one plain `def`")
        self.fdef = fdefs[0]
        self.globals = getattr(fn, "__globals__", {})
        self.lengths = lengths
        args = self.fdef.args
        if args.vararg or args.kwarg or args.kwonlyargs or getattr(args, "posonlyargs", []):
            raise self.err(self.fdef, "only plain positional arguments (params, inp, output[, memory]) are supported")
        if not 3 <= len(args.args) <= 4:
            raise self.err(self.fdef, "a body takes (params, inp, output[, memory])")
        self.arrays = {}
        for a, c in zip(args.args, _ARRAYS):
            self.arrays[a.arg] = _Array(c, c, lengths[c])
        self.views: dict[str, _Array] = {}
        self.types: dict[str, str] = {}
        self.tmp = 0

    # -- diagnostics -----------------------------------------------------------------------------------------------------------
    def err(self, node, why: str) -> NotImplementedError:
        line = self.first_line + getattr(node, "lineno", 1) - 1
        text = ast.get_source_segment(self.src, node) if hasattr(node, "lineno") else None
        text = (text or "").strip().splitlines()[0] if text else "?"
        return NotImplementedError(f"user block {self.bname}.{self.which} ({self.file}:{line}): {why}: `{text}` — the Python bodies of a "
                                   "user block are translated to device code (pycamset_amd/block_translate.py); write this body in the "
                                   "supported subset or give the block device_fun / device_jac strings (device_function_block)")

    # -- type inference (a local is int if every assignment to it is int-valued) ----------------------------------------------------
    def _infer(self):
        assigns = []          # (name, value node, kind): kind 'assign' (an augmented one as its BinOp) | 'loop'

        def targets(t, value):
            if isinstance(t, ast.Name):
                assigns.append((t.id, value, "assign"))
            elif isinstance(t, (ast.Tuple, ast.List)):
                if isinstance(value, (ast.Tuple, ast.List)) and len(value.elts) == len(t.elts):
                    for a, b in zip(t.elts, value.elts):
                        targets(a, b)
                else:
                    for a in t.elts:
                        targets(a, ast.Subscript(value=value, slice=ast.Constant(0), ctx=ast.Load()))
        for node in ast.walk(self.fdef):
            if isinstance(node, ast.Assign):
                for t in node.targets:
                    targets(t, node.value)
            elif isinstance(node, ast.AugAssign) and isinstance(node.target, ast.Name):
                assigns.append((node.target.id, ast.BinOp(left=ast.Name(node.target.id, ast.Load()), op=node.op, right=node.value), "assign"))
            elif isinstance(node, ast.For) and isinstance(node.target, ast.Name):
                assigns.append((node.target.id, None, "loop"))
        # views: a name bound to a slice / an array argument
        for name, value, kind in assigns:
            if kind == "assign" and self._is_array_expr(value):
                self.views[name] = None
        for name, value, kind in assigns:
            if name in self.arrays:
                continue
            if name not in self.views:
                self.types.setdefault(name, INT)
        changed = True
        while changed:
            changed = False
            for name, value, kind in assigns:
                if name in self.views or name in self.arrays or kind == "loop":
                    continue
                try:
                    t = self._type(value)
                except NotImplementedError:
                    t = DBL
                if t == DBL and self.types[name] != DBL:
                    self.types[name] = DBL
                    changed = True

    def _is_array_expr(self, v) -> bool:
        if isinstance(v, ast.Name):
            return v.id in self.arrays or v.id in self.views
        return isinstance(v, ast.Subscript) and isinstance(v.slice, ast.Slice) and self._is_array_expr(v.value)

    def _type(self, n) -> str:
        """Type of an expression without emitting it (for the inference pass)."""
        return self.expr(n)[1]

    # -- expressions: (C text, type) -----------------------------------------------------------------------------------------------
    def as_double(self, n) -> str:
        if isinstance(n, ast.Constant) and isinstance(n.value, (int, float)) and not isinstance(n.value, bool):
            return _lit(n.value, True)
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub) and isinstance(n.operand, ast.Constant) \
                and isinstance(n.operand.value, (int, float)) and not isinstance(n.operand.value, bool):
            return "(-" + _lit(n.operand.value, True) + ")"
        c, t = self.expr(n)
        return c if t == DBL else f"((double)({c}))"

    def as_int(self, n, why="an int is needed here") -> str:
        c, t = self.expr(n)
        if t == DBL:
            raise self.err(n, why)
        return c

    def cond(self, n) -> str:
        c, t = self.expr(n)
        return f"(({c}) != 0.0)" if t == DBL else f"({c})"

    def const_int(self, n):
        """The value of a constant int expression (literals, unary minus, frozen globals), else None."""
        if isinstance(n, ast.Constant) and isinstance(n.value, int) and not isinstance(n.value, bool):
            return n.value
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, (ast.USub, ast.UAdd)):
            v = self.const_int(n.operand)
            return None if v is None else (-v if isinstance(n.op, ast.USub) else v)
        if isinstance(n, ast.Name) and n.id not in self.types and n.id not in self.arrays and n.id not in self.views:
            g = self.globals.get(n.id)
            if isinstance(g, int) and not isinstance(g, bool):
                return g
        if isinstance(n, ast.BinOp) and isinstance(n.op, (ast.Add, ast.Sub, ast.Mult)):
            a, b = self.const_int(n.left), self.const_int(n.right)
            if a is not None and b is not None:
                return a + b if isinstance(n.op, ast.Add) else a - b if isinstance(n.op, ast.Sub) else a * b
        return None

    def array_of(self, n) -> _Array:
        if isinstance(n, ast.Name):
            if n.id in self.arrays:
                return self.arrays[n.id]
            if n.id in self.views:
                v = self.views[n.id]
                if v is None:
                    raise self.err(n, "this view is used before it is assigned")
                return v
        if isinstance(n, ast.Subscript) and isinstance(n.slice, ast.Slice):
            base = self.array_of(n.value)
            lo, hi = self.slice_bounds(n, base)
            return _Array(f"({base.cname} + {lo})" if lo else base.cname, base.base, hi - lo, base.offset + lo)
        raise self.err(n, "not an array")

    def slice_bounds(self, n, arr: _Array):
        s = n.slice
        if s.step is not None:
            raise self.err(n, "slices with a step are not supported")
        lo = 0 if s.lower is None else self.const_int(s.lower)
        hi = arr.length if s.upper is None else self.const_int(s.upper)
        if lo is None or hi is None:
            raise self.err(n, "slice bounds must be constants")
        lo, hi = (lo + arr.length if lo < 0 else lo), (hi + arr.length if hi < 0 else hi)
        lo, hi = max(0, min(lo, arr.length)), max(0, min(hi, arr.length))
        return lo, max(lo, hi)

    def index(self, n) -> str:
        """C lvalue / rvalue text of `array[i]`."""
        arr = self.array_of(n.value)
        k = self.const_int(n.slice)
        if k is not None:
            if k < 0:
                k += arr.length
            if not 0 <= k < arr.length:
                raise self.err(n, f"constant index out of range for an array of {arr.length}")
            return f"{arr.cname}[{k}]"
        return f"{arr.cname}[{self.as_int(n.slice, 'array indices must be ints')}]"

    def expr(self, n):
        if isinstance(n, ast.Constant):
            v = n.value
            if isinstance(v, bool):
                return ("1" if v else "0"), BOOL
            if isinstance(v, int):
                return _lit(v, False), INT
            if isinstance(v, float):
                return _lit(v, True), DBL
            raise self.err(n, "only int and float constants are supported")
        if isinstance(n, ast.Name):
            if n.id in self.types:
                return f"v_{n.id}", self.types[n.id]
            if n.id in self.arrays or n.id in self.views:
                raise self.err(n, "an array is only supported subscripted")
            g = self.globals.get(n.id, None)
            if isinstance(g, bool):
                return ("1" if g else "0"), BOOL
            if isinstance(g, (int, float)):
                return (_lit(g, False), INT) if isinstance(g, int) else (_lit(g, True), DBL)
            raise self.err(n, f"unknown name `{n.id}` (only locals, the four arguments and int / float module globals are supported)")
        if isinstance(n, ast.Attribute):
            if isinstance(n.value, ast.Name) and n.value.id in _MODULES and n.attr in _CONSTS:
                return _lit(_CONSTS[n.attr], True), DBL
            raise self.err(n, "unsupported attribute")
        if isinstance(n, ast.Subscript):
            if isinstance(n.slice, ast.Slice):
                raise self.err(n, "a slice is only supported as a view (`k = params[4:]`) or as the target of a scalar store")
            return self.index(n), DBL
        if isinstance(n, ast.UnaryOp):
            if isinstance(n.op, ast.Not):
                return f"(!{self.cond(n.operand)})", BOOL
            c, t = self.expr(n.operand)
            t = INT if t == BOOL else t
            if isinstance(n.op, ast.USub):
                return f"(-{c})", t
            if isinstance(n.op, ast.UAdd):
                return f"(+{c})", t
            raise self.err(n, "unsupported unary operator")
        if isinstance(n, ast.BinOp):
            return self.binop(n)
        if isinstance(n, ast.BoolOp):
            parts = []
            for v in n.values:
                c, t = self.expr(v)
                if t != BOOL:
                    raise self.err(n, "`and` / `or` are supported on comparisons and booleans only")
                parts.append(f"({c})")
            return "(" + (" && " if isinstance(n.op, ast.And) else " || ").join(parts) + ")", BOOL
        if isinstance(n, ast.Compare):
            terms, left = [], n.left
            for op, right in zip(n.ops, n.comparators):
                if type(op) not in _CMP:
                    raise self.err(n, "unsupported comparison")
                (lc, lt), (rc, rt) = self.expr(left), self.expr(right)
                if DBL in (lt, rt):
                    lc, rc = self.as_double(left), self.as_double(right)
                terms.append(f"({lc} {_CMP[type(op)]} {rc})")
                left = right
            return ("(" + " && ".join(terms) + ")" if len(terms) > 1 else terms[0]), BOOL
        if isinstance(n, ast.IfExp):
            (_, a), (_, b) = self.expr(n.body), self.expr(n.orelse)
            if DBL in (a, b):
                return f"({self.cond(n.test)} ? {self.as_double(n.body)} : {self.as_double(n.orelse)})", DBL
            return f"({self.cond(n.test)} ? {self.expr(n.body)[0]} : {self.expr(n.orelse)[0]})", (BOOL if a == b == BOOL else INT)
        if isinstance(n, ast.Call):
            return self.call(n)
        raise self.err(n, f"unsupported expression ({type(n).__name__})")

    def binop(self, n):
        (lc, lt), (rc, rt) = self.expr(n.left), self.expr(n.right)
        both_int = lt != DBL and rt != DBL
        op = type(n.op)
        if op in _ARITH:
            if both_int:
                return f"({lc} {_ARITH[op]} {rc})", INT
            return f"({self.as_double(n.left)} {_ARITH[op]} {self.as_double(n.right)})", DBL
        if op is ast.Div:
            return f"({self.as_double(n.left)} / {self.as_double(n.right)})", DBL
        if op in (ast.FloorDiv, ast.Mod):
            f = "floordiv" if op is ast.FloorDiv else "mod"
            if both_int:
                return f"pcs_py::{f}({lc}, {rc})", INT
            return f"pcs_py::{f}({self.as_double(n.left)}, {self.as_double(n.right)})", DBL
        if op is ast.Pow:
            k = self.const_int(n.right) if isinstance(n.right, (ast.Constant, ast.UnaryOp)) else None
            if k is not None and abs(k) <= MAX_SQUARING_EXPONENT:
                if k >= 0 and both_int:
                    return self._squaring(lc, k, INT), INT
                x = self.as_double(n.left)
                return (self._squaring(x, k, DBL) if k >= 0 else f"(1.0 / {self._squaring(x, -k, DBL)})"), DBL
            return f"pow({self.as_double(n.left)}, {self.as_double(n.right)})", DBL
        raise self.err(n, "unsupported operator")

    @staticmethod
    def _squaring(x: str, k: int, t: str) -> str:
        """x**k (k >= 0) as products by squaring: x is a side-effect-free expression, repeated textually."""
        if k == 0:
            return "1" if t == INT else "1.0"
        result, base = None, x
        while True:
            if k & 1:
                result = base if result is None else f"({result} * {base})"
            k >>= 1
            if not k:
                return result
            base = f"({base} * {base})"

    def call(self, n):
        f = n.func
        if n.keywords:
            raise self.err(n, "keyword arguments are not supported")
        name = None
        if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id in _MODULES:
            name, mod = f.attr, f.value.id
        elif isinstance(f, ast.Name) and f.id in ("min", "max", "abs", "float", "int"):
            name, mod = f.id, None
        if name is None:
            raise self.err(n, "calls are limited to the math / numpy scalar functions, min, max, abs, float and int")
        args = n.args
        if name in ("float", "float64") and len(args) == 1 and (mod is None or mod != "math"):
            return self.as_double(args[0]), DBL
        if name == "int" and mod is None and len(args) == 1:
            c, t = self.expr(args[0])
            return (f"((int)({c}))" if t == DBL else c), INT
        if name in ("min", "max") and mod is None:
            if len(args) != 2:
                raise self.err(n, "min / max take exactly two arguments")
            ts = [self.expr(a)[1] for a in args]
            if DBL in ts:
                return f"pcs_py::{name}2({self.as_double(args[0])}, {self.as_double(args[1])})", DBL
            return f"pcs_py::{name}2({self.expr(args[0])[0]}, {self.expr(args[1])[0]})", INT
        if name == "abs" and mod is None:
            if len(args) != 1:
                raise self.err(n, "abs takes one argument")
            c, t = self.expr(args[0])
            return (f"fabs({c})", DBL) if t == DBL else (f"pcs_py::max2({c}, -({c}))", INT)
        if name in _FUNCS and not (mod == "math" and name in ("arcsin", "arccos", "arctan", "arctan2", "absolute", "abs")):
            cname, arity = _FUNCS[name]
            if len(args) != arity:
                raise self.err(n, f"{name} takes {arity} argument(s)")
            text = f"{cname}({', '.join(self.as_double(a) for a in args)})"
            if mod == "math" and name in ("floor", "ceil"):       # math.floor / math.ceil return ints in Python
                return f"((int){text})", INT
            return text, DBL
        raise self.err(n, f"`{mod + '.' if mod else ''}{name}` is not supported")

    # -- statements ----------------------------------------------------------------------------------------------------------------
    def new_tmp(self) -> str:
        self.tmp += 1
        return f"t_{self.tmp}"

    def store(self, target, value_c: str, value_t: str, node, ind: str) -> list:
        if isinstance(target, ast.Name):
            if target.id in self.arrays or target.id in self.views:
                raise self.err(node, "an array argument or a slice view cannot be re-bound")
            t = self.types[target.id]
            if t == DBL and value_t != DBL:
                value_c = f"((double)({value_c}))"
            elif t != DBL and value_t == DBL:
                raise self.err(node, "a double assigned to an int local")
            return [f"{ind}v_{target.id} = {value_c};"]
        if isinstance(target, ast.Subscript):
            if isinstance(target.slice, ast.Slice):
                arr = self.array_of(target)
                self._check_writable(arr, node)
                if value_t != DBL:
                    value_c = f"((double)({value_c}))"
                q = self.new_tmp()
                return [f"{ind}#pragma unroll", f"{ind}for (int {q} = 0; {q} < {arr.length}; ++{q}) {arr.cname}[{q}] = {value_c};"]
            arr = self.array_of(target.value)
            self._check_writable(arr, node)
            if value_t != DBL:
                value_c = f"((double)({value_c}))"
            return [f"{ind}{self.index(target)} = {value_c};"]
        if isinstance(target, ast.Attribute):
            raise self.err(node, "attribute stores are not supported")
        raise self.err(node, "unsupported assignment target")

    def _check_writable(self, arr: _Array, node):
        if not arr.writable:
            raise self.err(node, "the block's params and inp are read-only")

    def assign(self, node, targets, value, ind: str) -> list:
        out = []
        for tgt in targets:
            if isinstance(tgt, ast.Name) and tgt.id in self.views:      # a slice view: a pointer with an offset
                if self.views[tgt.id] is not None or ind != "    ":
                    raise self.err(node, "a slice view is assigned once, at the top level of the body")
                arr = self.array_of(value)
                self.views[tgt.id] = _Array(f"w_{tgt.id}", arr.base, arr.length, arr.offset)
                out.append(f"{ind}{'' if arr.writable else 'const '}double *const w_{tgt.id} = {arr.cname};")
                continue
            if isinstance(tgt, (ast.Tuple, ast.List)):
                if isinstance(value, (ast.Tuple, ast.List)):
                    elts = value.elts
                elif self._is_array_expr(value):
                    arr = self.array_of(value)
                    elts = [ast.Subscript(value=value, slice=ast.Constant(i), ctx=ast.Load()) for i in range(arr.length)]
                    for e in elts:
                        ast.copy_location(e, value)
                        ast.copy_location(e.slice, value)
                else:
                    raise self.err(node, "only tuples and array slices can be unpacked")
                if len(elts) != len(tgt.elts):
                    raise self.err(node, "unpacking needs as many values as targets")
                temps = []
                for e in elts:               # Python evaluates the whole right-hand side first (`a, b = b, a`)
                    c, t = self.expr(e)
                    q = self.new_tmp()
                    ctype = "double" if t == DBL else "int"
                    out.append(f"{ind}const {ctype} {q} = {c};")
                    temps.append((q, t))
                for sub, (q, t) in zip(tgt.elts, temps):
                    if isinstance(sub, (ast.Tuple, ast.List, ast.Starred)):
                        raise self.err(node, "nested unpacking is not supported")
                    out += self.store(sub, q, t, node, ind)
                continue
            if isinstance(value, (ast.Tuple, ast.List)):
                raise self.err(node, "tuples and lists are only supported in unpacking assignments")
            c, t = self.expr(value)
            out += self.store(tgt, c, t, node, ind)
        return out

    def stmts(self, body, ind: str) -> list:
        out = []
        for s in body:
            out += self.stmt(s, ind)
        return out

    def stmt(self, s, ind: str) -> list:
        if isinstance(s, ast.Expr) and isinstance(s.value, ast.Constant) and isinstance(s.value.value, str):
            return []                                             # a docstring / a string used as a comment
        if isinstance(s, ast.Expr):
            self.expr(s.value)                                    # a call to another function is named as such
            raise self.err(s, "a bare expression does nothing")
        if isinstance(s, ast.Assign):
            return self.assign(s, s.targets, s.value, ind)
        if isinstance(s, ast.AugAssign):
            if isinstance(s.target, ast.Subscript) and isinstance(s.target.slice, ast.Slice):
                raise self.err(s, "augmented slice stores are not supported")
            if not isinstance(s.target, (ast.Name, ast.Subscript)):
                raise self.err(s, "unsupported augmented-assignment target")
            load = ast.copy_location(ast.Name(s.target.id, ast.Load()), s) if isinstance(s.target, ast.Name) else \
                ast.copy_location(ast.Subscript(value=s.target.value, slice=s.target.slice, ctx=ast.Load()), s)
            c, t = self.binop(ast.copy_location(ast.BinOp(left=load, op=s.op, right=s.value), s))
            return self.store(s.target, c, t, s, ind)
        if isinstance(s, ast.If):
            out = [f"{ind}if {self.cond(s.test)} {{"] + self.stmts(s.body, ind + "    ")
            if s.orelse:
                out += [f"{ind}}} else {{"] + self.stmts(s.orelse, ind + "    ")
            return out + [f"{ind}}}"]
        if isinstance(s, ast.For):
            return self.for_range(s, ind)
        if isinstance(s, ast.Pass):
            return []
        if isinstance(s, ast.Return):
            if s.value is not None and not (isinstance(s.value, ast.Constant) and s.value.value is None):
                raise self.err(s, "a body returns nothing (it writes `output`)")
            return [f"{ind}return;"]
        if isinstance(s, ast.Break):
            return [f"{ind}break;"]
        if isinstance(s, ast.Continue):
            return [f"{ind}continue;"]
        what = {ast.While: "`while` loops", ast.With: "`with`", ast.Try: "`try`", ast.FunctionDef: "nested functions",
                ast.Delete: "`del`", ast.Global: "`global`", ast.Nonlocal: "`nonlocal`", ast.AnnAssign: "annotated assignments"}.get(type(s))
        raise self.err(s, (what + " are not supported") if what else f"unsupported statement ({type(s).__name__})")

    def for_range(self, s, ind: str) -> list:
        it = s.iter
        if s.orelse:
            raise self.err(s, "`for ... else` is not supported")
        if not (isinstance(it, ast.Call) and isinstance(it.func, ast.Name) and it.func.id == "range" and 1 <= len(it.args) <= 3 and not it.keywords):
            raise self.err(s, "only `for ... in range(...)` loops are supported")
        if not isinstance(s.target, ast.Name):
            raise self.err(s, "the loop variable must be a name")
        a = it.args
        start, stop, step = (ast.Constant(0), a[0], ast.Constant(1)) if len(a) == 1 else (a[0], a[1], ast.Constant(1) if len(a) == 2 else a[2])
        consts = [self.const_int(x) for x in (start, stop, step)]
        k = self.new_tmp()
        var = s.target.id
        inner = [f"{ind}    v_{var} = {k};"] + self.stmts(s.body, ind + "    ")
        if all(c is not None for c in consts):
            c0, c1, c2 = consts
            if c2 == 0:
                raise self.err(s, "range() step must not be zero")
            return [f"{ind}#pragma unroll", f"{ind}for (int {k} = {c0}; {k} {'<' if c2 > 0 else '>'} {c1}; {k} += {c2}) {{"] + inner + [f"{ind}}}"]
        c0, c1, c2 = (self.as_int(x, "range() bounds must be ints") for x in (start, stop, step))
        b, st = self.new_tmp(), self.new_tmp()
        return [f"{ind}{{", f"{ind}const int {b} = {c1}, {st} = {c2};",
                f"{ind}for (int {k} = {c0}; {st} > 0 ? {k} < {b} : {k} > {b}; {k} += {st}) {{"] + inner + [f"{ind}}}", f"{ind}}}"]

    # -- whole body ----------------------------------------------------------------------------------------------------------------
    def translate(self) -> str:
        self._infer()
        for node in ast.walk(self.fdef):
            if isinstance(node, (ast.ListComp, ast.SetComp, ast.DictComp, ast.GeneratorExp, ast.Lambda, ast.Dict, ast.Set, ast.Starred,
                                 ast.Yield, ast.YieldFrom, ast.Await, ast.JoinedStr)):
                raise self.err(node, f"{type(node).__name__} is not supported")
        body = self.fdef.body
        code = self.stmts(body, "    ")
        decls = []
        for name, t in self.types.items():
            if name in self.views:
                continue
            decls.append(f"    {'double' if t == DBL else 'int'} v_{name} = {'0.0' if t == DBL else '0'};")
        memlen = self.lengths["mem"]
        head = [f"    // translated from {self.bname}.{self.which} ({os.path.basename(self.file)}:{self.first_line}) by pycamset_amd/block_translate.py"]
        if len(self.fdef.args.args) == 4:
            head.append(f"    double mem[{memlen}] = {{}};   // `memory`: max(1, array_memory) doubles, zeroed")
            head.append("    (void)mem;")
        return "\n".join(head + decls + code)


def _lengths(block, which: str) -> dict:
    npar, nin, nout = int(block.params.n_params), int(block.num_inp), int(block.num_out)
    inp = 3 if bool(getattr(block, "template", False)) and nin == 0 else nin
    out = nout if which == "compute_fun" else nout * (npar + nin)
    return {"params": npar, "inp": inp, "out": out, "mem": max(1, int(getattr(block, "array_memory", 0) or 0))}


def translate_body(block, which: str) -> str:
    """The C++ statements of ``which`` ('compute_fun' | 'compute_jac') of a Python-bodied block."""
    fn = body_function(block, which)
    if fn is None:
        raise NotImplementedError(f"user block {type(block).__name__} has no Python {which}")
    try:
        return _Translator(block, which, fn, _lengths(block, which)).translate()
    except (OSError, TypeError, SyntaxError) as e:
        raise NotImplementedError(f"user block {type(block).__name__}.{which}: its source cannot be read ({e})") from None
    except RecursionError:
        raise NotImplementedError(f"user block {type(block).__name__}.{which}: expression nesting too deep") from None


def translate_block(block) -> tuple[str, str]:
    """(device_fun, device_jac) of a Python-bodied user block."""
    return translate_body(block, "compute_fun"), translate_body(block, "compute_jac")
