"""The fold of history tapes, restated in numpy (include/elmk.h "history"; k_history.hip) - for the cell rows of the river stages
(ELMState.cell_history_add_row), where a sample is the row itself: no map, no fill, every cell a sample.

    SUM, AVG   acc = acc + v, from -0.0 (IEEE's exact additive identity: -0.0 + x == x for every x, -0.0 included)
    MAX        acc = v if (v > acc or v != v) else acc, from -inf: a NaN sticks
    MIN        the mirror, from +inf
    INST       acc = v: the last sample
    AVG is divided by the sample count once, when it is read: one correctly rounded division.

Every operation is one IEEE operation per element and sample, so the device's accumulators are these bit for bit (which NaN an
operation on a NaN returns is the one thing IEEE leaves open).
"""
import numpy as np

AVG, SUM, MAX, MIN, INST = range(5)  # ELMK_HIST_*
OPS = {"avg": AVG, "sum": SUM, "max": MAX, "min": MIN, "inst": INST}


def _op(op):
    return OPS[op] if isinstance(op, str) else int(op)


def init_value(op):
    """What a reset leaves in an accumulator of `op` (INST: a NaN that is never read before a sample)."""
    return {AVG: -0.0, SUM: -0.0, MAX: -np.inf, MIN: np.inf, INST: np.nan}[_op(op)]


def fold(op, acc, v):
    """One sample v folded into the accumulators acc (float64 arrays of one shape): the new accumulators."""
    op = _op(op)
    acc, v = np.asarray(acc, np.float64), np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        if op in (AVG, SUM):
            return acc + v
        if op == MAX:
            return np.where((v > acc) | (v != v), v, acc)
        if op == MIN:
            return np.where((v < acc) | (v != v), v, acc)
    if op != INST:
        raise ValueError(f"unknown history op {op}")
    return v.copy()


def finalize(op, acc, count):
    """What history_read returns for accumulators acc after `count` samples: acc / count for AVG, acc otherwise."""
    with np.errstate(all="ignore"):
        return np.asarray(acc, np.float64) / np.float64(count) if _op(op) == AVG else np.array(acc, np.float64)


def fold_cell_rows(op, samples, raw=False):
    """The result of a cell-row entry of `op` over `samples` - the row's values [ncells] after every step, in step order, as
    routing_read / irrigation_supply_read return them: float64 [ncells].  raw: the accumulators (AVG undivided)."""
    samples = [np.asarray(s, np.float64) for s in samples]
    if not samples:
        raise ValueError("fold_cell_rows: a tape without samples has no result")
    acc = np.full(samples[0].shape, init_value(op))
    for v in samples:
        if v.shape != acc.shape:
            raise ValueError("fold_cell_rows: samples of different shapes")
        acc = fold(op, acc, v)
    return acc if raw else finalize(op, acc, len(samples))
