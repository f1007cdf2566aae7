"""Cases of tests/golden/coreset_metric.npz (make_coreset_metric_golden.py): the reference's CoreSet(metric=...) under
the metrics other than "euclidean".  Poses are regenerated from the seeds on both sides (cases.coreset_arrays: pool poses
rounded to float32, labeled poses float64); the file stores results only."""
from collections import OrderedDict

import cases

# a golden case is admissible only if the reference's own top two min_distances differ by more than this (relative) at
# every greedy step: six orders above the 4.4e-16 by which two correct cosine evaluations differ
MIN_GAP = 1e-9

METRICS = ("manhattan", "cosine", "chebyshev")
ALIAS_OF = {"l1": "manhattan", "cityblock": "manhattan"}  # alias cases: the same picks and bits as the base metric
SHAPES = OrderedDict(
    n64_l5_j19=dict(seed=61, n=64, l=5, j=19, root=2, select=10),
    n1000_l200_j42=dict(seed=62, n=1000, l=200, j=42, root=21, select=20),
    n50000_l200_j19=dict(seed=63, n=50000, l=200, j=19, root=2, select=100),
)
ALIAS_SHAPE = "n64_l5_j19"
STORES_MIN_DISTANCES = ("n64_l5_j19", "n1000_l200_j42")  # (the 50 000-row vector would not fit the committed-file limit)


def coreset_metric_cases():
    """name "<metric>/<shape>" -> dict(metric, shape, seed, n, l, j, root, select)."""
    out = OrderedDict()
    for m in METRICS:
        for shape, c in SHAPES.items():
            out[m + "/" + shape] = dict(c, metric=m, shape=shape)
    for m in ALIAS_OF:
        out[m + "/" + ALIAS_SHAPE] = dict(SHAPES[ALIAS_SHAPE], metric=m, shape=ALIAS_SHAPE)
    return out


def arrays(c):
    """pool (n, J, 3) float32, labeled (l, J, 4) float64."""
    return cases.coreset_arrays(c)


def build(c):
    """(sal_dict, al_dict) as the reference sees them."""
    return cases.build_coreset_case(c)
