"""The rule of msnv_pcoa and msnv_pcoa_file (include/msnv.h) in numpy: ape::pcoa(correction = "none") by two-sided cyclic Jacobi in round-robin
order.  Vectorised per step, with the same fp64 operations in the same order as csrc/pcoa_k.hip (numpy's elementwise arithmetic is one operation
per element and never contracts), so the device is compared with it bit for bit; what the model is worth is checked in tests/test_pcoa_model.py
against answers known without it and against numpy.linalg.eigh."""
import numpy as np

import pammodel

EPS = 2.0 ** -52
CUT = float(np.sqrt(np.float64(EPS)))
MAX_SWEEPS = 64
OK, TOO_FEW_AXES = 0, 1


def seqsum(a, axis):
    """The sequential fp64 sum along an axis, first element first."""
    return np.take(np.add.accumulate(np.asarray(a, dtype=np.float64), axis=axis), -1, axis=axis)


def centre(d):
    """Gower centring.  Returns B (exactly symmetric: the cells i <= j mirrored) and its trace, summed sequentially."""
    d = np.asarray(d, dtype=np.float64)
    n = d.shape[0]
    a = -0.5 * (d * d)
    r = seqsum(a, 1) / np.float64(n)
    g = seqsum(r, 0) / np.float64(n)
    b = ((a - r[:, None]) - r[None, :]) + g
    up = np.triu_indices(n, 1)
    b[up[1], up[0]] = b[up]                                        # the mirror: the expression is not bit-symmetric in i and j
    return b, float(seqsum(np.diag(b), 0))


def step_pairs(n, r):
    """Step r of a sweep over n indices: the slots in order, each (p, q) with p < q; q == n marks the bye of an odd n (its only index is p)."""
    m = n + (n & 1)
    slots = [(m - 1, r)] + [((r + i) % (m - 1), (r - i) % (m - 1)) for i in range(1, m // 2)]
    return [(min(a, b), max(a, b)) for a, b in slots]


def params(a, p, q, tol):
    """t, c, s and the rotates flag of the pairs (p[i], q[i])."""
    apq = a[p, q]
    rot = np.abs(apq) > tol
    with np.errstate(all="ignore"):
        theta = (a[q, q] - a[p, p]) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
    return np.where(rot, t, 0.0), np.where(rot, c, 1.0), np.where(rot, s, 0.0), rot


def apply_step(a, v, pairs, tol):
    """One step on a and v in place.  Returns the number of pairs that rotated."""
    n = a.shape[0]
    bye = [p for p, q in pairs if q >= n]
    full = [(p, q) for p, q in pairs if q < n]                     # the bye is slot 0: every full pair comes behind it
    if not full:
        return 0
    p, q = np.array([x[0] for x in full]), np.array([x[1] for x in full])
    t, c, s, rot = params(a, p, q, tol)
    cj, sj, ci, si = c[None, :], s[None, :], c[:, None], s[:, None]
    w, x, y, z = a[np.ix_(p, p)], a[np.ix_(p, q)], a[np.ix_(q, p)], a[np.ix_(q, q)]
    w1, x1 = cj * w - sj * x, sj * w + cj * x                      # columns first, with the column pair's c and s
    y1, z1 = cj * y - sj * z, sj * y + cj * z
    w2, y2 = ci * w1 - si * y1, si * w1 + ci * y1                  # then rows, with the row pair's
    x2, z2 = ci * x1 - si * z1, si * x1 + ci * z1
    app, aqq, apq = a[p, p], a[q, q], a[p, q]
    new_pp, new_qq = app - t * apq, aqq + t * apq
    bye_rows = None
    if bye:
        bw, bx = a[bye[0], p], a[bye[0], q]
        bye_rows = (c * bw - s * bx, s * bw + c * bx)
    up = np.triu_indices(len(full), 1)                             # the blocks I < J, written to themselves and to their mirrors
    pi, qi, pj, qj = p[up[0]], q[up[0]], p[up[1]], q[up[1]]
    a[pi, pj] = w2[up]; a[pj, pi] = w2[up]
    a[pi, qj] = x2[up]; a[qj, pi] = x2[up]
    a[qi, pj] = y2[up]; a[pj, qi] = y2[up]
    a[qi, qj] = z2[up]; a[qj, qi] = z2[up]
    a[p, p], a[q, q] = new_pp, new_qq
    a[p[rot], q[rot]] = 0.0
    a[q[rot], p[rot]] = 0.0
    if bye:
        a[bye[0], p] = bye_rows[0]; a[p, bye[0]] = bye_rows[0]
        a[bye[0], q] = bye_rows[1]; a[q, bye[0]] = bye_rows[1]
    vp, vq = v[:, p], v[:, q]
    v[:, p], v[:, q] = cj * vp - sj * vq, sj * vp + cj * vq
    return int(rot.sum())


def jacobi(b):
    """Returns (the diagonal, V, sweeps, rotations) of the solve of the symmetric matrix b."""
    a = np.array(b, dtype=np.float64)
    n = a.shape[0]
    v = np.eye(n)
    tol = EPS * np.abs(a).max()
    m = n + (n & 1)
    sweeps = rotations = 0
    while True:
        if sweeps == MAX_SWEEPS:
            raise RuntimeError("the Jacobi solve of %d samples has not settled after %d sweeps" % (n, sweeps))
        rotated = sum(apply_step(a, v, step_pairs(n, r), tol) for r in range(m - 1))
        sweeps += 1
        rotations += rotated
        if rotated == 0:
            return np.diag(a).copy(), v, sweeps, rotations


def pcoa(d, n_axes=2, solved=None):
    """msnv_pcoa: a dict of eig, rel_eig, axis_pct, vectors [n x n_axes], status, sweeps, rotations, k, n_negative.  solved: centre(d) + jacobi(b)
    where a caller has them already."""
    if solved is None:
        b, trace = centre(d)
        solved = (b, trace) + jacobi(b)
    _, trace, lam, v, sweeps, rotations = solved
    n = len(lam)
    order = np.argsort(-lam, kind="stable")                        # descending; equal values in ascending diagonal position
    eig = lam[order]
    eig = np.where(np.abs(eig) < CUT, 0.0, eig)
    k = int((eig > CUT).sum())
    pos = np.where(eig > 0.0, eig, 0.0)
    with np.errstate(all="ignore"):
        rel = eig / np.float64(trace)
        pct = pos / seqsum(pos, 0) * 100.0
    vectors = np.full((n, n_axes), np.nan)
    for a in range(min(k, n_axes)):
        col = v[:, order[a]]
        top = int(np.argmax(np.abs(col)))                          # the first of equals
        x = col * np.sqrt(eig[a])
        vectors[:, a] = -x if col[top] < 0.0 else x
    return {"eig": eig, "rel_eig": rel, "axis_pct": pct, "vectors": vectors, "status": TOO_FEW_AXES if k < 2 else OK, "sweeps": sweeps,
            "rotations": rotations, "k": k, "n_negative": int((eig < -CUT).sum())}


def fmt(v):
    return "NaN" if v != v else "Inf" if v == np.inf else "-Inf" if v == -np.inf else "%.15g" % v


def r_column(text, column):
    """A table as write.table(sep = '\\t', quote = F) prints it -> {row name: the cell of `column`, as text}."""
    lines = [ln for ln in text.split("\n") if ln]
    col = lines[0].split("\t").index(column)
    return {f[0]: f[col + 1] for f in (ln.split("\t") for ln in lines[1:])}


def outliers_removed(d):
    """removeOutliersFromDistMatrixMinDissim as tests/pammodel.py's cluster_files has it: the indices that stay."""
    d = np.asarray(d, dtype=np.float64)
    n_all = d.shape[0]
    mind = (d + np.where(np.eye(n_all, dtype=bool), np.inf, 0.0)).min(axis=1)
    mean, sd = pammodel.r_mean(mind), pammodel.r_sd(mind)
    hi, lo = mean + 3 * sd, mean - 3 * sd
    keep = [i for i in range(n_all) if not (mind[i] > hi or mind[i] < lo)]
    return keep if 0 < n_all - len(keep) <= 5 else list(range(n_all))


def pcoa_files(names, d, species, clustering_text, composition_text=None):
    """msnv_pcoa_file.  Returns (files: name -> text, info: status, sweeps, rotations, k, n_negative, n_samples, n_outliers)."""
    d = np.asarray(d, dtype=np.float64)
    qc = outliers_removed(d)
    res = pcoa(d[np.ix_(qc, qc)], 2)
    clust = r_column(clustering_text, "clust")
    homog = r_column(composition_text, "freq_data_sample_10_90") if composition_text is not None else {}
    files = {species + "_mann_pcoa_eig.tab": "Eigenvalues\tRelative_eig\taxisPercent\n" + "".join(
        "%d\t%s\t%s\t%s\n" % (a + 1, fmt(res["eig"][a]), fmt(res["rel_eig"][a]), fmt(res["axis_pct"][a])) for a in range(len(qc)))}
    if res["status"] == OK:
        text = "Axis.1\tAxis.2\tpropFreqHomog\tclust\n"
        for a, i in enumerate(qc):
            h = homog.get(names[i], "NA")
            text += "%s\t%s\t%s\t%s\t%s\n" % (names[i], fmt(res["vectors"][a, 0]), fmt(res["vectors"][a, 1]), h if h == "NA" else fmt(float(h)),
                                             clust.get(names[i], "NA"))
        files[species + "_mann_pcoa_proj.tab"] = text
    info = {key: res[key] for key in ("status", "sweeps", "rotations", "k", "n_negative")}
    info.update(n_samples=len(qc), n_outliers=len(names) - len(qc))
    return files, info
