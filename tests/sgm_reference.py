"""NumPy restatement of the semi-global matcher's rule (include/pcs_hip.h, pcs_stereo_sgm; csrc/ba_stereo_sgm.hpp).  Everything is integer
arithmetic: the device is held to bit-equality with ``match``.  ``match_loops`` states the same rule pixel by pixel and path by path,
straight from the definitions, and is compared with ``match`` on a small crop.  The finish, the right-anchored winner, the reprojection
and the compaction are those of tests/stereo_reference.py."""
import numpy as np

from tests.stereo_reference import BIG, LEFT_RIGHT, NO_DR, NOT_STRICT, UNIQUENESS, VALIDITY, _finish, compact, reproject, right_disparity  # noqa: F401

DIRECTIONS = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]   # (dy, dx); the first four are paths = 4


def census(I, cw, ch):
    """-> (descriptor uint64 (H, W), inside bool (H, W)): one bit per window position other than the centre, 1 iff that neighbour is less
    than the centre; 0 where the window leaves the image."""
    I = np.asarray(I).astype(np.int64)
    H, W = I.shape
    rw, rh = cw // 2, ch // 2
    desc = np.zeros((H, W), dtype=np.uint64)
    inside = np.zeros((H, W), dtype=bool)
    if H < ch or W < cw:
        return desc, inside
    inside[rh:H - rh, rw:W - rw] = True
    centre = I[rh:H - rh, rw:W - rw]
    bits = np.zeros(centre.shape, dtype=np.uint64)
    for j in range(-rh, rh + 1):
        for i in range(-rw, rw + 1):
            if i == 0 and j == 0:
                continue
            nb = I[rh + j:H - rh + j, rw + i:W - rw + i]
            bits = (bits << np.uint64(1)) | (nb < centre).astype(np.uint64)
    desc[rh:H - rh, rw:W - rw] = bits
    return desc, inside


census_transform = census   # `match` takes the window as census=


def popcount(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)


def cost_volume(cL, inL, cR, inR, min_disp, D):
    """-> C (D, H, W) int64 and its domain (D, H, W) bool: C[k, y, x] = popcount(cL(y, x) xor cR(y, x - d)), d = min_disp + k."""
    H, W = cL.shape
    C = np.zeros((D, H, W), dtype=np.int64)
    ok = np.zeros((D, H, W), dtype=bool)
    for k in range(D):
        d = min_disp + k
        lo, hi = max(0, d), min(W, W + d)   # left columns x with 0 <= x - d < W
        if hi > lo:
            C[k][:, lo:hi] = popcount(cL[:, lo:hi] ^ cR[:, lo - d:hi - d])
            ok[k][:, lo:hi] = inL[:, lo:hi] & inR[:, lo - d:hi - d]
    return np.where(ok, C, 0), ok


def strict_rectangle(W, H, min_disp, D, cw, ch):
    """-> (ys0, ys1, xs0, xs1), ends exclusive and never below their starts."""
    rw, rh = cw // 2, ch // 2
    xs0 = rw + max(min_disp + D - 1, 0)
    return rh, max(H - rh, rh), xs0, max(W - rw + min(min_disp, 0), xs0)


def _step(prev, C, p1, p2):
    """One step of the recurrence for any number of lines: prev, C (..., D) -> L (..., D)."""
    M = prev.min(axis=-1, keepdims=True)
    lo = np.concatenate([np.full_like(prev[..., :1], BIG), prev[..., :-1]], axis=-1)   # L(d - 1); omitted at the end of the range
    hi = np.concatenate([prev[..., 1:], np.full_like(prev[..., :1], BIG)], axis=-1)
    return C + np.minimum(np.minimum(prev, M + p2), np.minimum(lo, hi) + p1) - M


def aggregate(Cs, p1, p2, paths):
    """Cs (Hs, Ws, D): the costs on the strict rectangle.  -> S (Hs, Ws, D), the sum of L_r over the directions.  One Python step per
    row or column of the rectangle, every line and disparity of it at once."""
    Hs, Ws, D = Cs.shape
    S = np.zeros_like(Cs)
    for dy, dx in DIRECTIONS[:paths]:
        L = np.empty_like(Cs)
        if dy == 0:
            cols = range(Ws) if dx > 0 else range(Ws - 1, -1, -1)
            for n, x in enumerate(cols):
                L[:, x] = Cs[:, x] if n == 0 else _step(L[:, x - dx], Cs[:, x], p1, p2)
        else:
            rows = range(Hs) if dy > 0 else range(Hs - 1, -1, -1)
            for n, y in enumerate(rows):
                if n == 0:
                    L[y] = Cs[y]
                    continue
                xs = np.arange(Ws)
                src = xs - dx
                has = (src >= 0) & (src < Ws)   # the predecessor lies in the rectangle; else the path starts here
                stepped = _step(L[y - dy][np.clip(src, 0, Ws - 1)], Cs[y], p1, p2)
                L[y] = np.where(has[:, None], stepped, Cs[y])
        S += L
    return S


def match(L, R, num_disp, census=(9, 7), min_disp=0, p1=8, p2=32, paths=8, uniqueness_ratio=15, lr_max_diff=-1, valid=None):
    """-> dict(disp int16, cost int32, status uint8, d_star, offset, strict, C, ok, m, p, S) for one pair (H, W); S (D, H, W) is 0 outside
    the strict rectangle."""
    D, (cw, ch) = int(num_disp), census
    cL, inL = census_transform(L, cw, ch)
    cR, inR = census_transform(R, cw, ch)
    H, W = cL.shape
    C, ok = cost_volume(cL, inL, cR, inR, min_disp, D)
    strict = ok.all(axis=0)
    ys0, ys1, xs0, xs1 = strict_rectangle(W, H, min_disp, D, cw, ch)
    rect = np.zeros((H, W), dtype=bool)
    rect[ys0:ys1, xs0:xs1] = True
    assert np.array_equal(rect, strict)
    S = np.zeros((D, H, W), dtype=np.int64)
    if strict.any():
        S[:, ys0:ys1, xs0:xs1] = aggregate(np.ascontiguousarray(C[:, ys0:ys1, xs0:xs1].transpose(1, 2, 0)), p1, p2, paths).transpose(2, 0, 1)
    Sm = np.where(strict[None], S, BIG)
    k_star = np.argmin(Sm, axis=0)   # the first, i.e. the smallest d, of the smallest S
    S_star = np.take_along_axis(Sm, k_star[None], axis=0)[0]
    d_star = min_disp + k_star
    status = np.zeros((H, W), dtype=np.int64)
    ks = np.arange(D)[:, None, None]
    if uniqueness_ratio > 0:
        far = np.abs(ks - k_star[None]) >= 2
        c2 = np.where(far, Sm, BIG).min(axis=0)
        status |= np.where((c2 < BIG) & (100 * c2 <= (100 + uniqueness_ratio) * S_star), UNIQUENESS, 0)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    xr = np.clip(xs - d_star, 0, W - 1)   # in range on every strict pixel
    if lr_max_diff >= 0:
        d_R = right_disparity(Sm, min_disp)
        status |= np.where(np.abs(d_star - d_R[ys, xr]) > lr_max_diff, LEFT_RIGHT, 0)
    if valid is not None:
        vL, vR = (np.asarray(v) for v in valid)
        status |= np.where((vL == 0) | (vR[ys, xr] == 0), VALIDITY, 0)
    interior = (k_star > 0) & (k_star < D - 1)
    m = np.take_along_axis(S, np.clip(k_star - 1, 0, D - 1)[None], axis=0)[0]
    p = np.take_along_axis(S, np.clip(k_star + 1, 0, D - 1)[None], axis=0)[0]
    offset = _finish(np.where(strict, S_star, 0), m, p, interior)
    status = np.where(strict, status, NOT_STRICT)
    disp = np.where(status == 0, 16 * d_star + offset, 16 * (min_disp - 1))
    cost = np.where(strict, S_star, -1)
    return dict(disp=disp.astype(np.int16), cost=cost.astype(np.int32), status=status.astype(np.uint8), d_star=d_star, offset=np.where(strict, offset, 0), strict=strict,
                C=C, ok=ok, m=m, p=p, S=S)


def match_stack(Ls, Rs, *args, valid=None, **kw):
    """``match`` over (n, H, W) stacks -> (disp, cost, status) stacks."""
    outs = [match(Ls[i], Rs[i], *args, valid=None if valid is None else (valid[0][i], valid[1][i]), **kw) for i in range(len(Ls))]
    return tuple(np.stack([o[k] for o in outs]) for k in ("disp", "cost", "status"))


def match_loops(L, R, num_disp, census=(9, 7), min_disp=0, p1=8, p2=32, paths=8, uniqueness_ratio=15, lr_max_diff=-1, valid=None):
    """The rule pixel by pixel and path by path, every term from its definition.  -> (disp, cost, status, S dict)."""
    D, (cw, ch) = int(num_disp), census
    rw, rh = cw // 2, ch // 2
    I = [np.asarray(L).astype(int), np.asarray(R).astype(int)]
    H, W = I[0].shape
    ds = list(range(min_disp, min_disp + D))

    def inside(y, x):
        return rh <= y <= H - 1 - rh and rw <= x <= W - 1 - rw

    def descriptor(im, y, x):
        return [int(im[y + j, x + i] < im[y, x]) for j in range(-rh, rh + 1) for i in range(-rw, rw + 1) if (i, j) != (0, 0)]

    def C(y, x, d):
        return sum(a != b for a, b in zip(descriptor(I[0], y, x), descriptor(I[1], y, x - d)))

    def is_strict(y, x):
        return 0 <= y < H and 0 <= x < W and all(inside(y, x) and 0 <= x - d < W and inside(y, x - d) for d in ds)

    memo = {}

    def path(y, x, dy, dx):
        """L_r(p, .) as a list over the range, from the path's start up to p."""
        start = (y, x)
        while is_strict(start[0] - dy, start[1] - dx):
            start = (start[0] - dy, start[1] - dx)
        q, prev = start, None
        while True:
            key = (q, dy, dx)
            if key not in memo:
                cs = [C(q[0], q[1], d) for d in ds]
                if prev is None:
                    memo[key] = cs
                else:
                    M = min(prev)
                    cur = []
                    for k in range(D):
                        terms = [prev[k], M + p2]
                        if k > 0:
                            terms.append(prev[k - 1] + p1)
                        if k < D - 1:
                            terms.append(prev[k + 1] + p1)
                        cur.append(cs[k] + min(terms) - M)
                    memo[key] = cur
            prev = memo[key]
            if q == (y, x):
                return prev
            q = (q[0] + dy, q[1] + dx)

    S = {}
    for y in range(H):
        for x in range(W):
            if is_strict(y, x):
                Ls = [path(y, x, dy, dx) for dy, dx in DIRECTIONS[:paths]]
                S[(y, x)] = [sum(Lr[k] for Lr in Ls) for k in range(D)]

    def d_right(y, x2):
        best = None
        for k, d in enumerate(ds):
            if (y, x2 + d) in S and (best is None or S[(y, x2 + d)][k] < best[0]):
                best = (S[(y, x2 + d)][k], d)
        return best[1]

    disp = np.full((H, W), 16 * (min_disp - 1), dtype=np.int16)
    cst = np.full((H, W), -1, dtype=np.int32)
    status = np.full((H, W), NOT_STRICT, dtype=np.uint8)
    for (y, x), s in S.items():
        s_star = min(s)
        k = s.index(s_star)
        d_star = ds[k]
        st = 0
        if uniqueness_ratio > 0 and any(abs(j - k) >= 2 and 100 * s[j] <= (100 + uniqueness_ratio) * s_star for j in range(D)):
            st |= UNIQUENESS
        if lr_max_diff >= 0 and abs(d_star - d_right(y, x - d_star)) > lr_max_diff:
            st |= LEFT_RIGHT
        if valid is not None and (valid[0][y, x] == 0 or valid[1][y, x - d_star] == 0):
            st |= VALIDITY
        off = 0
        if 0 < k < D - 1:
            den = 2 * (s[k - 1] + s[k + 1] - 2 * s_star)
            if den != 0:
                off = (32 * (s[k - 1] - s[k + 1]) + den) // (2 * den)   # Python's // floors
        cst[y, x], status[y, x] = s_star, st
        if st == 0:
            disp[y, x] = 16 * d_star + off
    return disp, cst, status, S
