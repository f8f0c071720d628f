"""Inputs shared by tests/test_hclust_model.py and tests/test_gpu_hclust.py: hand-worked trees, seeded matrices (`manhattan`: tie-free; `integer`:
many equal cells and zero distances between distinct samples, tests/pamcases.py), the model's results for them (computed once per process, never
written to) and the comparison with scipy's linkage that both files make on the same terms."""
import numpy as np

import hclustmodel as model
import pamcases

KINDS = ("manhattan", "integer")
THREADS = 256                                                      # csrc/device.h: HCLUST_THREADS, the lanes of a task's workgroup
# two members (one step), 3 .. 5, a wavefront of columns and one more or fewer, the workgroup's lanes and one more or fewer
MODEL_SIZES = (2, 3, 4, 5, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1)
SCIPY_SIZES = (THREADS + 1, 2 * THREADS + 1)
LDS_SWITCH = 48 * 1024 // 24 + 1                                   # 2049 members: 24 bytes of LDS each, the first size above the 48 KiB a launch gets unasked
CAP = 4096                                                         # csrc/device.h: CLUSTER_MAX_SAMPLES
SCIPY_NAMES = {model.AVERAGE: "average", model.COMPLETE: "complete", model.SINGLE: "single", model.MCQUITTY: "weighted"}


def square(m, cells):
    d = np.zeros((m, m))
    for (i, j), v in cells.items():
        d[i, j] = d[j, i] = v
    return d


# name -> (matrix, {method: (merge, height, order)}); every number worked by hand from the rule of include/msnv.h
LINE4 = square(4, {(0, 1): 2, (0, 2): 6, (0, 3): 10, (1, 2): 5, (1, 3): 9, (2, 3): 4})
FIVE = square(5, {(0, 1): 1, (0, 2): 4, (0, 3): 8, (0, 4): 16, (1, 2): 3, (1, 3): 9, (1, 4): 15, (2, 3): 10, (2, 4): 14, (3, 4): 20})
TIE_A = square(4, {(0, 1): 5, (0, 2): 6, (0, 3): 1, (1, 2): 1, (1, 3): 7, (2, 3): 8})        # d03 = d12: the smaller a, (0, 3), goes first
TIE_B = square(4, {(0, 1): 5, (0, 2): 1, (0, 3): 1, (1, 2): 6, (1, 3): 7, (2, 3): 8})        # d02 = d03: the smaller b, (0, 2), goes first
# (1, 3) merge first; single link then sets W[0][1] = min(9, 3) = 3 = row 0's nearest distance, so far held at column 2: column 1 takes over
UNDERCUT = square(4, {(0, 1): 9, (0, 2): 3, (0, 3): 3, (1, 2): 8, (1, 3): 1, (2, 3): 7})
_TWO_PAIRS = [[-1, -2], [-3, -4], [1, 2]]
_CHAIN5 = [[-1, -2], [-3, 1], [-4, 2], [-5, 3]]
HAND = {
    "line4": (LINE4, {model.AVERAGE: (_TWO_PAIRS, [2, 4, 7.5], [0, 1, 2, 3]), model.COMPLETE: (_TWO_PAIRS, [2, 4, 10], [0, 1, 2, 3]),
                      model.SINGLE: (_TWO_PAIRS, [2, 4, 5], [0, 1, 2, 3]), model.MCQUITTY: (_TWO_PAIRS, [2, 4, 7.5], [0, 1, 2, 3])}),
    "five": (FIVE, {model.AVERAGE: (_CHAIN5, [1, 3.5, 9, 16.25], [4, 3, 2, 0, 1]), model.COMPLETE: (_CHAIN5, [1, 4, 10, 20], [4, 3, 2, 0, 1]),
                    model.SINGLE: (_CHAIN5, [1, 3, 8, 14], [4, 3, 2, 0, 1]), model.MCQUITTY: (_CHAIN5, [1, 3.5, 9.25, 17.375], [4, 3, 2, 0, 1])}),
    "tie_a": (TIE_A, {model.COMPLETE: ([[-1, -4], [-2, -3], [1, 2]], [1, 1, 8], [0, 3, 1, 2])}),
    "tie_b": (TIE_B, {model.SINGLE: ([[-1, -3], [-4, 1], [-2, 2]], [1, 1, 5], [1, 3, 0, 2])}),
    "undercut": (UNDERCUT, {model.SINGLE: ([[-2, -4], [-1, 1], [-3, 2]], [1, 3, 3], [2, 0, 1, 3])}),
}


def matrix(kind, m):
    """manhattan: the summed absolute differences of unrounded profiles around three centres, one coordinate at a time (the same order for (i, j)
    and (j, i): exactly symmetric) -- no two cells are equal (tie_free; the rounded tables of tests/pamcases.py repeat a cell now and then).
    integer: pamcases.integer_dist."""
    if kind == "manhattan":
        rng = np.random.default_rng(300 + m)
        dims = 60 if m <= 600 else 8 if m <= 2049 else 4
        centres = rng.uniform(0, 100, size=(3, dims))
        p = centres[np.arange(m) % 3] + rng.normal(0, 30.0, size=(m, dims))
        d = np.zeros((m, m))
        for c in range(dims):
            d += np.abs(p[:, c, None] - p[None, :, c])
        return d
    return pamcases.integer_dist(m, 400 + m)


def tie_free(d):
    cells = d[np.triu_indices(d.shape[0], 1)]
    return np.unique(cells).size == cells.size


def same_nearest_column(m):
    """Every row's nearest column is the last active one, so the column that leaves in a step was the nearest of every row."""
    i = np.arange(m)
    d = 2.0 * m - np.maximum(i[:, None], i[None, :]) + 0.001 * np.minimum(i[:, None], i[None, :])
    d[i, i] = 0.0
    return d


_want = {}


def want(kind, m, method):
    """hclustmodel.hclust of every sample of matrix(kind, m)."""
    key = (kind, m, method)
    if key not in _want:
        d = same_nearest_column(m) if kind == "same_nearest" else matrix(kind, m)
        res = model.hclust(d, np.arange(m), method)
        for v in res.values():
            v.setflags(write=False)
        _want[key] = res
    return _want[key]


def members_by_step(m, merge):
    sets = {}
    for s in range(1, m):
        sets[s] = frozenset().union(*[frozenset([-e - 1]) if e < 0 else sets[e] for e in np.asarray(merge)[s - 1].tolist()])
    return [sets[s] for s in range(1, m)]


def check_against_scipy(d, merge, height, method):
    """On a tie-free matrix: the same member set at every step in the same order; complete and single heights bit-equal, average and weighted ones
    within 4 (m - 1) 2^-53 relative (three roundings per nested update, at most m - 1 updates deep).  Returns the largest relative difference."""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    m = d.shape[0]
    z = linkage(squareform(d, checks=False), method=SCIPY_NAMES[method])
    sets = {}
    for s in range(m - 1):
        sets[m + s] = frozenset().union(*[frozenset([int(e)]) if e < m else sets[int(e)] for e in z[s, :2]])
    assert members_by_step(m, merge) == [sets[m + s] for s in range(m - 1)]
    rel = float(np.max(np.abs(height - z[:, 2]) / z[:, 2]))
    if method in (model.COMPLETE, model.SINGLE):
        assert height.tobytes() == z[:, 2].tobytes()
    else:
        assert rel <= 4 * (m - 1) * 2.0 ** -53
    return rel


def check_tree(m, res):
    """What holds on any matrix: heights non-decreasing, merge a tree, order a permutation in which every row's two clusters are adjacent runs, the
    first one on the left."""
    assert (np.diff(res["height"]) >= 0).all()
    assert model.is_tree(m, res["merge"])
    order = res["order"].tolist()
    assert sorted(order) == list(range(m))
    place = {p: i for i, p in enumerate(order)}
    sets = {}
    for s in range(1, m):
        left, right = [frozenset([-e - 1]) if e < 0 else sets[e] for e in res["merge"][s - 1].tolist()]
        pl, pr = sorted(place[p] for p in left), sorted(place[p] for p in right)
        assert pl == list(range(pl[0], pl[0] + len(pl))) and pr == list(range(pl[-1] + 1, pl[-1] + 1 + len(pr)))
        sets[s] = left | right


def stage_samples():
    """45 samples in two planted groups (tests/pcoacases.py): names and their Manhattan distances."""
    import pcoacases
    names, table, order = pcoacases.stage_samples()
    return names, table, order, pamcases.manhattan(table)
