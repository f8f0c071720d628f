"""The row order of subpopr's report heatmaps, restated in numpy from include/msnv.h (msnv_hclust_tasks, msnv_heatmap_order, msnv_heatmap_file): the
yardstick the device is compared with bit for bit (tests/test_gpu_hclust.py).  Checked itself in tests/test_hclust_model.py against hand-worked
trees and scipy's linkage.

The search for the minimum is naive: np.argmin over the row-major upper triangle of the active cells, which returns the first of equal values --
the smallest a, then the smallest b.  Every update is numpy's element-wise fp64 arithmetic, one rounding per operation."""
import numpy as np

from pcoamodel import fmt, r_column

AVERAGE, COMPLETE, SINGLE, MCQUITTY = range(4)
METHODS = (AVERAGE, COMPLETE, SINGLE, MCQUITTY)
METHOD_NAMES = {AVERAGE: "average", COMPLETE: "complete", SINGLE: "single", MCQUITTY: "mcquitty"}
OK, NO_DISCOVERY = range(2)


def steps(d, idx, method):
    """The m - 1 steps of a task: lists a, b (positions in idx, a < b) and h."""
    idx = np.asarray(idx, dtype=np.int64)
    m = len(idx)
    w = np.asarray(d, dtype=np.float64)[np.ix_(idx, idx)].copy()
    size = np.ones(m)
    active = np.ones(m, dtype=bool)
    upper = np.triu(np.ones((m, m), dtype=bool), 1)
    out_a, out_b, out_h = [], [], []
    for _ in range(m - 1):
        cand = np.where(upper & active[:, None] & active[None, :], w, np.inf)
        a, b = divmod(int(np.argmin(cand)), m)
        out_a.append(a)
        out_b.append(b)
        out_h.append(w[a, b])
        k = np.flatnonzero(active)
        k = k[(k != a) & (k != b)]
        x, y = w[k, a], w[k, b]
        if method == AVERAGE:
            v = (size[a] * x + size[b] * y) / (size[a] + size[b])
        elif method == COMPLETE:
            v = np.maximum(x, y)
        elif method == SINGLE:
            v = np.minimum(x, y)
        else:
            v = 0.5 * x + 0.5 * y
        w[k, a] = v
        w[a, k] = v
        size[a] += size[b]
        active[b] = False
    return out_a, out_b, np.array(out_h, dtype=np.float64)


def leaves(m, children):
    """The leaves of the tree left to right (0-based positions); children[s - 1] = (left, right) of the node made at step s, in hc$merge's labels."""
    out, stack = [], [m - 1]
    while stack:
        e = stack.pop()
        if e < 0:
            out.append(-e - 1)
        else:
            stack.append(children[e - 1][1])
            stack.append(children[e - 1][0])
    return np.array(out, dtype=np.int32)


def tree(m, a, b):
    """R's hc$merge [m - 1, 2] and hc$order (0-based) from the steps."""
    label = [-(p + 1) for p in range(m)]
    merge = np.zeros((m - 1, 2), dtype=np.int32)
    for s in range(1, m):
        la, lb = label[a[s - 1]], label[b[s - 1]]
        if (la > 0 and lb < 0) or (la > 0 and lb > 0 and lb < la):
            la, lb = lb, la
        merge[s - 1] = (la, lb)
        label[a[s - 1]] = s
    return merge, leaves(m, merge.tolist())


def hclust(d, idx, method):
    a, b, h = steps(d, idx, method)
    merge, order = tree(len(idx), a, b)
    return {"merge": merge, "height": h, "order": order}


def is_tree(m, merge):
    merge = np.asarray(merge).reshape(-1, 2)
    if m < 2 or merge.shape[0] != m - 1:
        return False
    seen = set()
    for s in range(1, m):
        for e in merge[s - 1].tolist():
            if e == 0 or e in seen or e < -m or e >= s:
                return False
            seen.add(e)
    return True


def reorder(merge, weights):
    """reorder(as.dendrogram(hc), weights) with agglo.FUN = sum, then order.dendrogram: (order, the value of every node by step)."""
    weights = np.asarray(weights, dtype=np.float64)
    m = len(weights)
    value = [None] * m
    kids = []

    def of(e):
        return weights[-e - 1] if e < 0 else value[e]
    for s in range(1, m):
        left, right = (int(e) for e in merge[s - 1])
        if of(left) > of(right):
            left, right = right, left
        kids.append((left, right))
        value[s] = np.float64(np.longdouble(of(left)) + np.longdouble(of(right)))
    return leaves(m, kids), kids, value


def row_means(sub):
    """R's rowMeans: a long double sum over ascending columns, divided by the number of columns, rounded to double."""
    sub = np.asarray(sub, dtype=np.float64)
    return (np.cumsum(sub.astype(np.longdouble), axis=1)[:, -1] / np.longdouble(sub.shape[1])).astype(np.float64)


def heatmap_files(names, d, species, used_text=None, clustering_text=None):
    """msnv_heatmap_file.  used_text: <species>_mann_distMatrixUsedForClustMedoidDefns.txt (None: absent), clustering_text likewise.  Returns
    (files: name -> text, info: status, n_samples, n_discovery, have_clustering)."""
    d = np.asarray(d, dtype=np.float64)
    at = {nm: i for i, nm in enumerate(names)}
    trees = [("all", list(range(len(names))), AVERAGE)]
    if used_text is not None:
        header = used_text.split("\n")[0].rstrip("\r")
        sub = [at[nm] for nm in header.split("\t")] if header else []
        if len(sub) >= 2:
            trees.append(("discovery", sub, COMPLETE))
    discovery = set(trees[1][1]) if len(trees) > 1 else set()
    clust = r_column(clustering_text, "clust") if clustering_text is not None else {}
    files = {}
    for which, members, method in trees:
        res = hclust(d, members, method)
        m = len(members)
        files["%s_mann_hclust_%s.tab" % (species, which)] = "merge1\tmerge2\theight\n" + "".join(
            "%d\t%d\t%d\t%s\n" % (s, res["merge"][s - 1, 0], res["merge"][s - 1, 1], fmt(res["height"][s - 1])) for s in range(1, m))
        heat = reorder(res["merge"], row_means(d[np.ix_(members, members)]))[0]
        pos = np.zeros(m, dtype=np.int64)
        pos[res["order"]] = np.arange(m)
        files["%s_mann_heatmap_%s.tab" % (species, which)] = "index\thclustPos\tinDiscoverySubset\tclust\n" + "".join(
            "%s\t%d\t%d\t%s\t%s\n" % (names[members[p]], p + 1, pos[p] + 1, "TRUE" if members[p] in discovery else "FALSE", clust.get(names[members[p]], "NA"))
            for p in heat.tolist())
    info = {"status": OK if len(trees) > 1 else NO_DISCOVERY, "n_samples": len(names), "n_discovery": len(trees[1][1]) if len(trees) > 1 else 0,
            "have_clustering": clustering_text is not None}
    return files, info
