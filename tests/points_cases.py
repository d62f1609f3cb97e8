"""The inputs of the point-series tests, host and device (include/elmk.h "point series"): the lists at the sizes the record kernel can
go wrong at - one point, a wave of 64, a wave and one, a workgroup of 256 and one -, the column row with the values a gather has to carry
bit for bit, the output map of the gridded test (a cell of 2100 terms: several passes of 64; cells of exactly 64 and 65 terms; empty
cells), a synthetic state of every stored type for the host test, and the straight loop the restatement is compared with."""
import numpy as np

from elmkernels_amd import points as pt

NCOL = 5003  # no multiple of 64: the level stride is padded
BASE_COLUMNS = (0, 5002, 17, 17, 4096, 3)  # unsorted, with a duplicate, first and last column
SIZES = (1, 64, 65, 257)
NCELL_ROWS = 1001  # the cell stride is padded to 1024
BASE_CELLS = (0, 1000, 63, 64)
NCELL_GRID = 70
BIG, EXACT, EXACT1 = 7, 11, 12  # the cells of 2100, 64 and 65 terms
EMPTY = (0, 33, 69)
NAN_PAYLOAD = np.array([0x7FF8000000ABC000], np.uint64).view(np.float64)[0]  # a quiet NaN whose payload survives fp32
SPECIALS = (NAN_PAYLOAD, -0.0, float("inf"), float("-inf"))
FILL = 1.0e36


def column_list(n, ncols=NCOL, base=BASE_COLUMNS, seed=5):
    """n points: the base list (from its second point on where n is smaller: the last column), then random columns with repeats."""
    more = np.random.default_rng(seed + n).integers(0, ncols, max(n, len(base)))
    a = np.concatenate([np.array(base, np.int64), more])
    return a[1:2] if n == 1 else a[:n]


def cell_list(n, ncells=NCELL_ROWS, base=BASE_CELLS):
    return column_list(n, ncells, base, seed=11)


def plant_specials(x, at, f32=False):
    """x with SPECIALS written round-robin into the positions `at` (a copy; rounded to the stored fp32 where the build stores that)."""
    x = np.array(x, np.float64)
    at = np.unique(np.asarray(at))
    x[at] = np.resize(np.array(SPECIALS), at.size)
    return x.astype(np.float32).astype(np.float64) if f32 else x


def grid_map(ncols=NCOL, ncells=NCELL_GRID, seed=21):
    """A CSR map of ncols columns over ncells cells: cell BIG holds 2100 terms, EXACT exactly 64, EXACT1 exactly 65, the cells EMPTY none,
    the rest 1 .. 90; columns drawn with repeats, weights in (0, 1.5).  Returns (ptr, col, w)."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 91, ncells)
    cnt[BIG], cnt[EXACT], cnt[EXACT1] = 2100, 64, 65
    cnt[list(EMPTY)] = 0
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col = rng.integers(0, ncols, int(ptr[-1])).astype(np.int32)
    return ptr, col, rng.uniform(0.01, 1.5, col.size)


def wide_row(n, seed):
    """Finite values over many decades of both signs (a sum in another order would differ)."""
    rng = np.random.default_rng(seed)
    return 10.0 ** rng.uniform(-30.0, 30.0, n) * rng.choice([-1.0, 1.0], n)


# ---- the host test's synthetic state -------------------------------------------------------------------------------------------------
def synthetic_rows(ncols=300, ncells=40, seed=3):
    """{name: row} of every stored type: two levels of a fp64 field, a fp32-stored row, int32, uint8, uint32, and a cell row; the
    specials stand in the fp64 and fp32 rows."""
    rng = np.random.default_rng(seed)
    at = np.arange(0, ncols, 37)
    f64a = plant_specials(wide_row(ncols, seed), at)
    f64z = plant_specials(wide_row(ncols, seed + 1), at + 1)
    f32 = plant_specials(rng.normal(size=ncols), at).astype(np.float32)
    return {"t_soisno/0": f64a, "t_soisno/last": f64z, "f32": f32, "snl": rng.integers(-5, 1, ncols).astype(np.int32),
            "veg_active": rng.integers(0, 2, ncols).astype(np.uint8), "err_flags": rng.integers(0, 2 ** 32, ncols, dtype=np.uint64).astype(np.uint32),
            "VOLR": plant_specials(wide_row(ncells, seed + 2), [0, ncells - 1])}


def loop_record(rows, lists, entries, map=None):
    """points.record, as a straight loop over the points in Python floats (a float64 product and sum per term)."""
    out = []
    for name, kind, how in entries:
        x = rows[name]
        v = np.empty(len(lists[kind]))
        for i, p in enumerate(lists[kind]):
            if how == pt.GATHER:
                v[i] = np.float64(x[p])
            else:
                ptr, col, w, fill = map
                acc = np.float64(fill)
                for q in range(ptr[p], ptr[p + 1]):
                    term = np.float64(w[q]) * np.float64(x[col[q]])
                    acc = term if q == ptr[p] else acc + term
                v[i] = acc
        out.append(v)
    return out


def words(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((words(a) == words(b)).all())
