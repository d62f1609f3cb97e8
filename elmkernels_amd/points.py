"""The point series, restated in numpy (include/elmk.h "point series", P0 - P9; k_points.hip): per-step records of chosen columns and
river cells.

    record(state_rows, lists, entries, map)   the values of one record, P1 and P2
    ring(total, max_records)                  the order of the held records, P3

An entry is one source sampled at the points of its list.  Here a source is a row, the way the device holds it: float64, float32 (a
fp64 field of libelmk_f32.so), int32, uint32 or uint8 [ncols], or float64 [ncells] for a cell row.  A sample is the stored value widened
to float64 - exact for every one of these types, NaN payloads, infinities and -0.0 included - and a gridded sample is
regrid.apply_aggregate's value of the widened row at that one cell: fill for a cell without terms, else the products w[p] * x[col[p]]
added in term order from the first product.
"""
import numpy as np

from . import regrid

COLUMNS, CELLS = range(2)  # ELMK_POINTS_COLUMNS, ELMK_POINTS_CELLS: the two lists
MAX_ENTRIES, MAX_POINTS = 64, 4096  # ELMK_POINTS_MAX_ENTRIES, ELMK_POINTS_MAX_POINTS (per list)
GATHER, GRIDDED = "gather", "gridded"


def widen(row):
    """A stored row as float64, P1: float64 as stored (bit for bit), float32 / int32 / uint32 / uint8 exactly."""
    a = np.asarray(row)
    if a.dtype not in (np.float64, np.float32, np.int32, np.uint32, np.uint8):
        raise ValueError(f"not a stored element type: {a.dtype}")
    return a if a.dtype == np.float64 else a.astype(np.float64)


def record(state_rows, lists, entries, map=None):
    """The values of one record.  state_rows: {name: row}; lists: (columns, cells), each a sequence of indices in any order, duplicates
    allowed; entries: [(name, kind, how)] with kind COLUMNS or CELLS - the list the entry samples - and how GATHER (values[i] =
    row[list[i]]) or GRIDDED (kind CELLS; values[i] = the aggregate of the column row over cell list[i]); map: (ptr, col, w, fill) of the
    output grid, needed by GRIDDED entries.  Returns one float64 array per entry, in list order."""
    out = []
    for name, kind, how in entries:
        idx = np.asarray(lists[kind], dtype=np.int64).reshape(-1)
        x = widen(state_rows[name])
        if how == GATHER:
            if idx.size and (idx.min() < 0 or idx.max() >= x.shape[-1]):
                raise ValueError(f"{name}: a point lies outside the row")
            v = np.empty(idx.size)
            v.view(np.uint64)[:] = np.ascontiguousarray(x).view(np.uint64)[idx]  # (bits, not values: a NaN keeps its payload)
            out.append(v)
        elif how == GRIDDED:
            if kind != CELLS or map is None:
                raise ValueError(f"{name}: a gridded entry samples the cells list through the output grid's map")
            ptr, col, w, fill = map
            out.append(np.ascontiguousarray(regrid.apply_aggregate(ptr, col, w, x, fill)[idx]))
        else:
            raise ValueError(f"{name}: unknown entry form {how!r}")
    return out


def ring(total, max_records):
    """P3: record r (0-based since the last reset) lands in slot r % max_records.  Returns (records, slots): the numbers of the held
    records, oldest first - what points_read and points_stamps index - and the slot of each; held = min(total, max_records)."""
    total, m = int(total), int(max_records)
    if m < 1 or total < 0:
        raise ValueError("need max_records >= 1 and total >= 0")
    held = min(total, m)
    records = np.arange(total - held, total, dtype=np.int64)
    return records, records % m
