"""NumPy restatement of the per-group residual statistics (include/pcs_hip.h pcs_stats_*, csrc/ba_groupstats.hpp): a plain loop over the
groups, ``np.median``, and the same exclusion of detections whose error is not finite.  ``e`` may be given (the device's own array) to
separate the selection from the rounding of e."""
import numpy as np

FIELDS = ("count", "n_nonfinite", "argmax", "sum_e", "sum_e2", "sum_ru", "sum_rv", "max_e", "median", "mad")
GROUPINGS = ("camera", "image", "key", "view", "overall")


def errors(resid):
    r = np.asarray(resid, dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.hypot(r[:, 0], r[:, 1])


def group_ids(cam, img, key, counts):
    """{grouping: (ids (n,), number of groups)} for the id columns of a table; the view of (c, i) is c * I + i."""
    C, I, K = counts
    cam, img, key = (np.asarray(a, dtype=np.int64) for a in (cam, img, key))
    return {"camera": (cam, C), "image": (img, I), "key": (key, K), "view": (cam * I + img, C * I), "overall": (np.zeros(cam.shape[0], dtype=np.int64), 1)}


def group_stats(resid, ids, n_groups, e=None):
    """-> {field: (n_groups,)} and, as 'abs', the sums of the absolute terms of the four sums (for the tolerance of a sum)."""
    r = np.asarray(resid, dtype=np.float64).reshape(-1, 2)
    e = errors(r) if e is None else np.asarray(e, dtype=np.float64)
    out = {f: np.full(n_groups, np.nan) for f in FIELDS[3:]}
    out.update({f: np.zeros(n_groups, dtype=np.int64) for f in FIELDS[:3]})
    out["abs"] = np.zeros((4, n_groups))
    for g in range(n_groups):
        rows = np.nonzero(ids == g)[0]                 # ascending table order
        fin = np.isfinite(e[rows])
        out["n_nonfinite"][g] = np.count_nonzero(~fin)
        rows = rows[fin]
        out["count"][g] = rows.size
        eg = e[rows]
        terms = (eg, eg * eg, r[rows, 0], r[rows, 1])
        for name, t in zip(("sum_e", "sum_e2", "sum_ru", "sum_rv"), terms):
            out[name][g] = t.sum()
        out["abs"][:, g] = [np.abs(t).sum() for t in terms]
        if rows.size == 0:
            out["argmax"][g] = -1
            continue
        out["max_e"][g] = eg.max()
        out["argmax"][g] = rows[np.argmax(eg)]         # the first of equal maxima: the lowest row
        out["median"][g] = np.median(eg)
        out["mad"][g] = np.median(np.abs(eg - out["median"][g]))
    return out


def all_group_stats(resid, cam, img, key, counts, e=None):
    return {name: group_stats(resid, ids, n, e) for name, (ids, n) in group_ids(cam, img, key, counts).items()}


def mad_score(values):
    """|v - median| / MAD over the non-NaN entries (NaN stays NaN): what ``diagnostics.mad_outliers`` compares with its threshold."""
    v = np.asarray(values, dtype=np.float64)
    ok = ~np.isnan(v)
    mdn = np.median(v[ok])
    return np.abs(v - mdn) / np.median(np.abs(v[ok] - mdn))
