"""What the restart size tests share (test_restart_plan_host.py, test_gpu_restart_sizes.py): a restatement of rst_plan of
elmkernels_amd/csrc/api_restart.cpp in plain Python - how an image is cut into staging chunks, the chunks into pieces, and how many
workgroups a piece's row gets -, the section table an image of a given context has (rst_layout restated, so that a size's property is
asserted without a GPU), the sizes the GPU tests run at with the property each was chosen for, and the element patterns and
poisons of those tests.  Asserts here carry a message: the module is not rewritten by pytest."""
import collections

import numpy as np

from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests.support import same

# the three constants of the plan, as in api_restart.cpp (test_restart_plan_host.py reads the source's and compares)
CHUNK = 64 << 20  # RST_CHUNK: bytes of image per staging chunk
BLOCK = 4096  # elements of the widest piece per workgroup of a row
NBX_CAP = 64  # most workgroups per row; a piece beyond NBX_CAP * BLOCK elements takes grid-stride trips
MAX_PIECES = 8192  # RST_MAX_PIECES: per chunk
THREADS = 256  # k_rst_pieces: elements per workgroup and trip
IMAGE_CLASSES = (st.CLASS_PROGNOSTIC, st.CLASS_SURFACE)

Piece = collections.namedtuple("Piece", "section level first count offset")  # offset: bytes from the chunk's lo
Chunk = collections.namedtuple("Chunk", "lo hi pieces nbx")


def plan(sections):
    """rst_plan: the chunks of an image with this section table (restart.parse(img)["sections"], or `layout`)."""
    chunks, pieces, start, end, maxn = [], None, 0, 0, 0

    def close():
        chunks.append(Chunk(start, end, pieces, int(min(NBX_CAP, max(1, (maxn + BLOCK - 1) // BLOCK)))))

    for s, S in enumerate(sections):
        es = R.ELEM[int(S["dtype"])].itemsize
        ext, base = int(S["extent"]), int(S["offset"])
        for lev in range(int(S["nlev"])):
            c = 0
            while c < ext:
                off = base + (lev * ext + c) * es
                if pieces is None or off + es > start + CHUNK or len(pieces) >= MAX_PIECES:
                    if pieces is not None:
                        close()
                    pieces, start, maxn = [], off, 0
                n = min(ext - c, (start + CHUNK - off) // es)
                pieces.append(Piece(s, lev, c, n, off - start))
                maxn = max(maxn, n)
                end = off + n * es
                c += n
    if pieces is not None:
        close()
    return chunks


def cuts(chunks):
    """The pieces that begin inside a row (first > 0): each is the second part of a row that a chunk boundary cuts."""
    return [p for ch in chunks for p in ch.pieces if p.first > 0]


def trips(count, nbx):
    """Grid-stride trips of the busiest workgroup of a piece of `count` elements under nbx workgroups."""
    return max(1, -(-count // (nbx * THREADS)))


# ---- the section table of a context (rst_layout) ---------------------------------------------------------------------------------------
DTYPE_CODE = {np.dtype(v): k for k, v in st.DTYPES.items()}
OPTIONAL_SECTIONS = {R.ALT_SECTION: 3, R.HYDROLOGY_SECTION: 2, R.IRRIGATION_SECTION: 2}  # one-level F64 column sections per kind


def image_fields():
    """[(name, field id, levels, numpy dtype)] of the fields an image holds, in id order."""
    ft = st.field_table()
    return sorted(((k, fid, nlev, np.dtype(dt)) for k, (fid, nlev, dt) in ft.items() if st.field_class(k) in IMAGE_CLASSES), key=lambda f: f[1])


def layout(ncols, history=(), accum=(), optional=()):
    """The section table (restart.SECTION, offsets filled in, checksums 0) of a context of ncols columns: history = [(levels, cells or
    None)] per entry in registration order, accum = [levels] per accumulator entry, optional = the kinds of OPTIONAL_SECTIONS enabled."""
    rows = [(R.FIELD, fid, nlev, DTYPE_CODE[dt], ncols) for _, fid, nlev, dt in image_fields()]
    rows += [(R.GRIDDED if cells else R.HISTORY, i, nlev, 0, cells or ncols) for i, (nlev, cells) in enumerate(history)]
    rows += [(R.ACCUM_SECTION, i, nlev, 0, ncols) for i, nlev in enumerate(accum)]
    rows += [(k, i, 1, 0, ncols) for k in sorted(optional) for i in range(OPTIONAL_SECTIONS[k])]
    sec = np.zeros(len(rows), R.SECTION)
    version = max([R.VERSION] + ([R.VERSION_ACCUM] if accum else []) + [dict(R.OPTIONAL)[k] for k in optional])
    off = R._align(R.HEADER.itemsize + (8 if version >= R.VERSION_ACCUM else 0) + len(history) * R.ENTRY.itemsize + len(accum) * R.ACCUM.itemsize +
                   len(rows) * R.SECTION.itemsize)
    for i, (kind, sid, nlev, dt, ext) in enumerate(rows):
        sec[i] = (kind, sid, nlev, dt, ext, off, 0)
        off = R._align(off + nlev * ext * R.ELEM[dt].itemsize)
    return sec, off


# ---- the sizes -------------------------------------------------------------------------------------------------------------------------
GRID_N = 70  # columns of the contexts whose gridded sections are wide
# cells of the output grid -> (nbx of the chunk, 256-element trips of a workgroup over the widest piece), which
# test_restart_plan_host.py asserts: the last size with one workgroup; two workgroups, the ninth trip holding one element; three;
# the cap reached, BLOCK elements each; the first size at which a workgroup goes beyond BLOCK elements; twice that and ragged
GRID_CELLS = {4096: (1, 16), 4097: (2, 9), 8193: (3, 11), 262144: (64, 16), 262145: (64, 17), 524288 + 300: (64, 33)}
GRID_CUT_CELLS = 420001  # a 20-level gridded section of 67.2 MB: a chunk boundary inside one of its rows (row stride 420032, not ld)
FIELD_N_SMALL = {4097: 2, 8193: 3}  # columns -> nbx of the field rows, one chunk
# 4 chunks, two cuts inside F64 rows and one inside a 4-byte row; plan() over 49 000 .. 52 000 finds that in 49 671 .. 49 721 only
FIELD_N_LARGE = 49703
LARGE_GCOL0 = 2**33 + 5


def grid_history(ncells, levels20=False):
    """The history entries of the gridded cases as `layout` takes them: GRID_ENTRIES, then the column entry."""
    return [(20 if levels20 and name == "t_soisno" else 1, ncells) for name, _ in (GRID_ENTRIES_CUT if levels20 else GRID_ENTRIES)] + [(1, None)]


GRID_ENTRIES = (("t_grnd", "avg"), ("t_grnd", "max"), ("t_grnd", "min"), ("t_grnd", "sum"))  # gridded, tape 0; one level
GRID_ENTRIES_CUT = (("t_soisno", "sum"), ("t_grnd", "max"))  # the 20-level entry first, so that the cut row has rows after it
LARGE_HISTORY = (("h2osoi_liq", "max"), ("t_grnd", "sum"))  # column entries of the large field case, tape 1: 20 levels and 1
LARGE_OPTIONAL = (R.ALT_SECTION, R.HYDROLOGY_SECTION, R.IRRIGATION_SECTION)


def large_layout(ncols):
    ft = st.field_table()
    return layout(ncols, [(ft[name][1], None) for name, _ in LARGE_HISTORY], [ft["t_grnd"][1]], LARGE_OPTIONAL)


# ---- element patterns --------------------------------------------------------------------------------------------------------------------
_M52 = np.uint64((1 << 52) - 1)
# planted F64 bit patterns: +-0, the smallest and the largest denormal, a negative denormal, +-inf, quiet NaNs of both signs with
# payloads, and 1e-40 and -3e-42, which are denormal once rounded to fp32 (no signalling NaN: the fp32-state build quiets them)
SPECIALS = np.array([0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x8000000000000400, 0x7FF0000000000000,
                     0xFFF0000000000000, 0x7FF8000000000123, 0xFFF800000000BEEF, 0x7FFC0DE000000000], np.uint64)
SPECIALS = np.concatenate([SPECIALS, np.array([1e-40, -3e-42]).view(np.uint64)])


def pattern(name, fid, nlev, dt, n, salt=0):
    """Field `name` as elmk_upload takes it ([n, nlev], or [n]): a hash of (field id, level, column), so that no two elements of the image
    agree and a piece one row, one workgroup or one chunk away from its place shows.  F64: mostly finite values inside the range of
    fp32, one in sixteen with any exponent at all (NaNs quieted), and SPECIALS at one column in 61; snl in 0 .. nlevsno."""
    col = np.arange(n, dtype=np.uint64)[:, None]
    lev = np.arange(nlev, dtype=np.uint64)[None, :]
    h = R.fmix64((np.uint64(fid + 1 + 1000 * salt) << np.uint64(44)) + (lev << np.uint64(36)) + col + np.uint64(0x9E3779B9))
    dt = np.dtype(dt)
    if dt == np.float64:
        sign = h & np.uint64(1 << 63)
        tame = sign | ((np.uint64(923) + ((h >> np.uint64(52)) & np.uint64(0xFF)) % np.uint64(200)) << np.uint64(52)) | (h & _M52)
        wild = np.where((h >> np.uint64(52)) & np.uint64(0x7FF) == np.uint64(0x7FF), h | np.uint64(1 << 51), h)
        bits = np.where(h & np.uint64(15) == np.uint64(3), wild, tame)
        k = (col + np.uint64(7) * lev + np.uint64(fid)) % np.uint64(61)
        bits = np.where(k < np.uint64(SPECIALS.size), SPECIALS[np.minimum(k, np.uint64(SPECIALS.size - 1)).astype(np.int64)], bits)
        out = bits.view(np.float64)
    elif name == "snl":
        out = (h % np.uint64(6)).astype(np.int32)
    elif dt == np.uint8:
        out = (h & np.uint64(0xFF)).astype(np.uint8)
    else:
        out = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(dt)
    return np.ascontiguousarray(out.reshape(n) if nlev == 1 else out)


def column_rows(n, k, salt=0):
    """Row k of a feature (an accumulator's values, altmax, ZWT, RATE ...): finite, distinct in every column and between rows."""
    return (R.fmix64(np.arange(n, dtype=np.uint64) + np.uint64((k + 1 + 100 * salt) << 40)) >> np.uint64(11)).astype(np.float64) * 2.0**-40 + k


def fill_pattern(D, salt=0, only_image=False):
    for name, (fid, nlev, dt) in D.fields.items():
        if not only_image or st.field_class(name) in IMAGE_CLASSES:
            D[name] = pattern(name, fid, nlev, dt, D.ncols, salt)


def with_section(img, p, i, data):
    """A copy of the image img (p = restart.parse(img)) with section i replaced by data and a matching checksum in the table, as
    restart.build would give it, patched in place: a few bytes instead of a rebuild of a large image."""
    out = img.copy()
    off = int(p["sections"][i]["offset"])
    out[off:off + data.nbytes] = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    word = 8 if int(p["header"]["version"]) >= R.VERSION_ACCUM else 0
    at = R.HEADER.itemsize + word + p["entries"].nbytes + p["accum"].nbytes + i * R.SECTION.itemsize + R.SECTION.fields["checksum"][1]
    g0 = 0 if int(p["sections"][i]["kind"]) == R.GRIDDED else int(p["header"]["gcol0"])
    out[at:at + 8] = np.frombuffer(np.uint64(R.checksum(data, g0)).tobytes(), np.uint8)
    ck = R.HEADER.fields["header_checksum"][1]
    out[ck:ck + 8] = np.frombuffer(np.uint64(R.header_checksum(out, int(p["header"]["header_bytes"]))).tobytes(), np.uint8)
    return out


def poison_fields(D):
    """Every field of the context, image fields included: NaN, or 3."""
    for name, (fid, nlev, dt) in D.fields.items():
        D.fill(name, np.nan if dt == np.float64 else 3.0)


def fields_of(D, image_only=False):
    return {k: D[k] for k in D.fields if not image_only or st.field_class(k) in IMAGE_CLASSES}


def assert_same_fields(a, b, what):
    for k in a:
        assert same(a[k], b[k]), f"{what}: field {k}"
