"""The regression tree of step 04's SUMS segmentation (VIDEO_SEGMENTATION_METHOD = 1), restated on the host without sklearn.

The reference fits DecisionTreeRegressor(max_depth=None, min_samples_leaf=leaf_min) to (x = 0 .. n - 1, y = the frame sums) and
compares the predictions with `!=` and `<` (video_segmenter.py:31-86), so a prediction has to come out bit for bit.  With one
feature whose values are all different every node is a range of frames; what has to be repeated is the ORDER of the float64
additions of the squared-error criterion:

  * a node's sum and sum of squares are added up sample by sample in the order the node's samples lie in at that moment: frame
    order for the root and for a left child, but r1, r2, .., r(k-1), r0 for a right child, because the parent's last partition
    step rotates the (sorted) right part by one and the child's totals are taken before its own sort;
  * the sum of the left part of a candidate split runs forward over the node's sorted samples;
  * for the winning split the left sum is taken once more, from whichever end is nearer -- from the far end it starts at the node's
    total and subtracts the right part's samples from the back, which by then lie in the rotated order;
  * a child's impurity is the one its parent computed for it, never recomputed.

np.cumsum adds sequentially (np.sum adds pairwise), so the running sums below are cumsum's.  The tree is tiny next to everything
else in the step (one feature, a few thousand points per lecture), so it stays on the host.
"""
import numpy as np

EPSILON = float(np.finfo(np.float64).eps)


def _running(values):
    """sequential float64 sum of `values` (0.0 for none)"""
    return float(np.cumsum(values)[-1]) if len(values) else 0.0


class SumsRegressor:
    """predict(X) of the fitted tree, X = frame numbers (any shape with one value per row, as the reference passes them)."""

    def __init__(self, leaf_starts, leaf_values, n):
        self.leaf_starts = np.asarray(leaf_starts, np.int64)     # first frame of every leaf, ascending
        self.leaf_values = np.asarray(leaf_values, np.float64)
        self.n = int(n)

    def predict(self, X):
        x = np.asarray(X, np.float64).reshape(len(X), -1)[:, 0]
        # the thresholds lie half way between two frames: frame f belongs to the last leaf that starts at or before it
        leaf = np.searchsorted(self.leaf_starts.astype(np.float64) - 0.5, x, side="left") - 1
        return self.leaf_values[np.clip(leaf, 0, len(self.leaf_values) - 1)]


def fit(all_sums, leaf_min):
    y = np.array(all_sums, dtype=np.float64)
    n = len(y)
    if n == 0:
        raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required")
    leaf_min = int(leaf_min)
    if leaf_min < 1:
        raise ValueError("min_samples_leaf must be at least 1, got %d" % leaf_min)
    sq = y * y
    leaf_starts, leaf_values = [], []
    todo = [(0, n, None, False)]                    # (first, one past last, impurity handed down, is a right child)
    while todo:
        a, b, impurity, rotated = todo.pop()
        m = b - a
        ys, qs = y[a:b], sq[a:b]
        if rotated:
            total = _running(np.concatenate([ys[1:], ys[:1]]))
            sq_total = _running(np.concatenate([qs[1:], qs[:1]]))
        else:
            total, sq_total = _running(ys), _running(qs)
        if impurity is None:
            impurity = sq_total / m - (total / m) ** 2.0
        if m < 2 or m < 2 * leaf_min or impurity <= EPSILON:
            leaf_starts.append(a)
            leaf_values.append(total / m)
            continue
        # candidates p = leaf_min .. m - leaf_min (samples on the left); the first jump, 0 -> leaf_min, is never nearer the end here
        left = np.cumsum(ys)[leaf_min - 1:m - leaf_min]
        p = np.arange(leaf_min, m - leaf_min + 1, dtype=np.float64)
        right = total - left
        with np.errstate(all="ignore"):
            proxy = left * left / p + right * right / (m - p)
        if np.isfinite(proxy).all():
            best = int(np.argmax(proxy))            # the first of equal maxima: a later one would have to be strictly larger
        else:
            best, best_value = -1, -np.inf
            for k, v in enumerate(proxy):
                if v > best_value:
                    best, best_value = k, v
        if best < 0:
            leaf_starts.append(a)
            leaf_values.append(total / m)
            continue
        p = leaf_min + best
        # the winning split once more: the left sum from the nearer end (the right part lies rotated by now)
        if p <= m - p:
            sum_left = _running(ys[:p])
        else:
            back = np.concatenate([ys[p:p + 1], ys[:p:-1]]) if p < m else ys[:0]
            sum_left = float(np.cumsum(np.concatenate([[total], -back]))[-1])
        sum_right = total - sum_left
        sq_left = _running(qs[:p])
        sq_right = sq_total - sq_left
        imp_left = sq_left / p - (sum_left / p) ** 2.0
        imp_right = sq_right / (m - p) - (sum_right / (m - p)) ** 2.0
        improvement = (m / n) * (impurity - ((m - p) / m) * imp_right - (p / m) * imp_left)
        if improvement + EPSILON < 0.0:
            leaf_starts.append(a)
            leaf_values.append(total / m)
            continue
        todo.append((a + p, b, imp_right, True))    # left child first: it is popped first
        todo.append((a, a + p, imp_left, False))
    return SumsRegressor(leaf_starts, leaf_values, n)
