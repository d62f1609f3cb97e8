"""Host codec of restart images (include/elmk.h "restart"), in numpy only: read, check, merge and cut the images that
elmk_restart_save writes, so that a run can restart with another column decomposition.

    img = S.restart_save(gcol0)              # one rank's columns
    full = restart.merge([img0, img1])       # adjacent column ranges -> one image; checksums add
    part = restart.slice(full, gcol0, n)     # columns [gcol0, gcol0 + n) for another rank; checksums recomputed
    restart.write(path, part); restart.read(path)

merge and slice refuse images with gridded history entries: per-rank partial cell accumulators do not survive a change of
decomposition under MAX and MIN.

An image holds exactly the optional kinds of its context, after the field and history sections and in this order, and its version is
the highest among them (OPTIONAL; version 1 without any, byte for byte as before the kinds existed):
  version 2, accumulated fields (elmk_accum_add): the word after the header counts the entries - present from version 2 on, 0 without
    entries -, their table (ACCUM: source, kind, destination, period, step count) follows the history entries, their value rows are
    sections of kind ACCUM_SECTION; parse returns the table under "accum", build takes it as `accum`, merge requires equal tables;
  version 3, active layer thickness (elmk_active_layer_enable): three column sections of kind ALT_SECTION (id 0, 1, 2: alt, altmax,
    altmax_lastyear; one level, F64);
  version 4, soil hydrology (elmk_soil_hydrology_enable): two column sections of kind HYDROLOGY_SECTION (id 0, 1: ZWT, WA; one level, F64).
  version 5, irrigation (elmk_irrigation_enable): two column sections of kind IRRIGATION_SECTION (id 0, 1: RATE, NLEFT; one level, F64).
  version 6, the routing state (ELMK_OPT_RESTART_CELLS on a context with the routing enabled): CELL sections of kind ROUTING_SECTION (id =
    ELMK_ROUTE_*: VOLR and QOUT_SUM always, WH and WT with the kinematic-wave scheme, WF with the inundation; one level, F64, extent = the
    routing's ncells, checksummed with g = the cell as GRIDDED sections are) and, with the river supply limit on, one of kind
    IRRSUP_SECTION (id = ELMK_IRRSUP_UNMET_SUM); a second 8-byte word after the accumulator-count word holds the routing's call count
    (int64): parse returns it under "routing_ncalls" (None below version 6), build takes it as `routing_ncalls`.  merge and slice refuse a
    version-6 image: cell data does not follow a column decomposition.
  version 7, the routing state of a context with the reservoirs on (elmk_routing_reservoir_enable): version 6 with two more
    ROUTING_SECTIONs, ELMK_ROUTE_RES and ELMK_ROUTE_KRLS, after WF.  The device saves and loads it; this module does not read it:
    parse, and with it verify, merge and slice, refuse a version-7 image by its version word, so it is never merged or sliced.
  version 8, the routing state of a context with the stream temperature on (elmk_routing_heat_enable): version 6 with two more
    ROUTING_SECTIONs, ELMK_ROUTE_TT and ELMK_ROUTE_TR, after WT.  The device saves and loads it; this module does not read it: its
    version word lies above MAX_VERSION, so parse, and with it verify, merge and slice, refuse it.
History entries over feature rows (elmk_column_history_add_row; include/elmk_restart.def): the entry's `field` holds row_field(family, which), a
value beyond every field id; its section is an ordinary HISTORY or GRIDDED section of one level and the version does not change.  merge
and slice carry such entries as they carry every entry; entry_row decodes one.
History entries over cell rows of the river stages (elmk_cell_history_add_row): `field` holds row_field(ROWS_NFAMILY + cell-row family,
which), `gridded` is CELL_ROW_ENTRY (2), `ncells` the routing's cells, and the accumulators are a GRIDDED section of one level and that
extent, checksummed with g = the cell; the version does not change.  merge and slice refuse an image that holds one, as they refuse
gridded entries: cell data does not follow a column decomposition.
build derives the version from the sections and `accum` it is given; merge and slice carry the sections as they carry every column section.
"""
import numpy as np

MAGIC = b"ELMKRST\0"
VERSION = 1  # of an image without accumulator entries
VERSION_ACCUM = 2  # of an image with accumulator entries
VERSION_ALT = 3  # of an image with the active layer thickness rows
VERSION_HYDROLOGY = 4  # of an image with the soil hydrology rows ZWT and WA
VERSION_IRRIGATION = 5  # of an image with the irrigation rows RATE and NLEFT
VERSION_ROUTING = 6  # of an image with the routing state (ELMK_OPT_RESTART_CELLS): cell sections, and the call count after the count word
VERSION_RESERVOIR = 7  # ... of a context with the reservoirs on: version 6 plus the ROUTING_SECTIONs RES and KRLS; refused by parse
VERSION_HEAT = 8  # ... of a context with the stream temperature on: version 6 plus the ROUTING_SECTIONs TT and TR; above MAX_VERSION, refused by parse
FIELD, HISTORY, GRIDDED, ACCUM_SECTION, ALT_SECTION, HYDROLOGY_SECTION, IRRIGATION_SECTION = 0, 1, 2, 3, 4, 5, 6  # ELMK_RESTART_*
ROUTING_SECTION, IRRSUP_SECTION = 7, 8  # (cell sections: extent = the routing's ncells, checksummed with g = the cell)
CELL_SECTIONS = (GRIDDED, ROUTING_SECTION, IRRSUP_SECTION)
# the optional kinds and the version that introduced each; from version 2 on the word after the header counts the accumulator entries
OPTIONAL = ((ACCUM_SECTION, VERSION_ACCUM), (ALT_SECTION, VERSION_ALT), (HYDROLOGY_SECTION, VERSION_HYDROLOGY),
            (IRRIGATION_SECTION, VERSION_IRRIGATION))
# the optional CELL kinds (the routing state), after the column kinds in an image, and the highest version parse accepts
OPTIONAL_CELLS = ((ROUTING_SECTION, VERSION_ROUTING), (IRRSUP_SECTION, VERSION_ROUTING))
MAX_VERSION = VERSION_ROUTING
ALIGN = 256
ROW_BASE = 0x40000000  # ELMK_RESTART_ROW_BASE
ROWS_ALT, ROWS_HYDROLOGY, ROWS_FROST, ROWS_WATER_BALANCE, ROWS_IRRIGATION = range(5)  # ELMK_ROWS_*
ROWS_NFAMILY = 5  # ELMK_ROWS_NFAMILY: a cell-row entry's family is ROWS_NFAMILY + CELL_ROWS_*
CELL_ROWS_ROUTING, CELL_ROWS_SUPPLY = range(2)  # ELMK_CELL_ROWS_*
GRIDDED_ENTRY, CELL_ROW_ENTRY = 1, 2  # elmk_restart_entry.gridded
HEADER = np.dtype([("magic", "S8"), ("version", "<u4"), ("real_bytes", "<u4"), ("schema_hash", "<u8"), ("gcol0", "<i8"),
                   ("ncols", "<i8"), ("tape_count", "<u8", (4,)), ("nentries", "<u4"), ("nsections", "<u4"),
                   ("header_bytes", "<u8"), ("total_bytes", "<u8"), ("header_checksum", "<u8")])
ENTRY = np.dtype([("tape", "<i4"), ("field", "<i4"), ("op", "<i4"), ("gridded", "<i4"), ("ncells", "<i8")])
SECTION = np.dtype([("kind", "<i4"), ("id", "<i4"), ("nlev", "<i4"), ("dtype", "<i4"), ("extent", "<i8"), ("offset", "<u8"),
                    ("checksum", "<u8")])
ACCUM = np.dtype([("src_field", "<i4"), ("kind", "<i4"), ("dst_field", "<i4"), ("pad", "<i4"), ("period", "<i8"), ("nsteps", "<u8")])
assert HEADER.itemsize == 104 and ENTRY.itemsize == 24 and SECTION.itemsize == 40 and ACCUM.itemsize == 32
ELEM = {0: np.dtype("<f8"), 1: np.dtype("<i4"), 2: np.dtype("u1"), 3: np.dtype("<u4")}  # elmk_dtype -> image element
_CK_OFF = HEADER.fields["header_checksum"][1]


class RestartError(ValueError):
    pass


def row_field(family, which):
    """ELMK_RESTART_ROW_FIELD: what elmk_restart_entry.field holds for a history entry over row `which` of feature family `family`."""
    return ROW_BASE + (int(family) << 16) + int(which)


def entry_row(field):
    """(family, which) of an entry over a feature row, or None for an entry over a state field."""
    field = int(field)
    return ((field - ROW_BASE) >> 16, (field - ROW_BASE) & 0xFFFF) if field >= ROW_BASE else None


def _version(sec, na):
    """An image's version: the highest among the optional kinds it holds (ACCUM_SECTION: with na > 0 accumulator entries), else 1."""
    return max((v for k, v in OPTIONAL + OPTIONAL_CELLS if (na > 0 if k == ACCUM_SECTION else bool(np.any(sec["kind"] == k)))), default=VERSION)


def _align(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


def fmix64(k):
    """murmur3's 64-bit finalizer, elementwise on uint64 (wrapping)."""
    k = np.asarray(k, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xFF51AFD7ED558CCD)
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xC4CEB9FE1A85EC53)
        k = k ^ (k >> np.uint64(33))
    return k


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 8:
        return a.view(np.uint64)
    if a.dtype.itemsize == 4:
        return a.view(np.uint32).astype(np.uint64)
    return a.astype(np.uint64)


def checksum(data, g0=0):
    """Checksum of a section [nlev, extent]: sum mod 2^64 of fmix64(bits ^ fmix64(g * 64 + lev + 1)), g = g0 + element index."""
    data = np.asarray(data)
    if data.ndim == 1:
        data = data[None, :]
    nlev, ext = data.shape
    pos = (np.uint64(g0) + np.arange(ext, dtype=np.uint64))[None, :] * np.uint64(64) + np.arange(nlev, dtype=np.uint64)[:, None] + np.uint64(1)
    return int(np.sum(fmix64(_bits(data) ^ fmix64(pos)), dtype=np.uint64))


def header_checksum(img, header_bytes):
    w = np.frombuffer(bytes(img[:header_bytes]), dtype="<u8").copy()
    w[_CK_OFF // 8] = 0
    return int(np.sum(fmix64(w ^ fmix64(np.arange(w.size, dtype=np.uint64) * np.uint64(64) + np.uint64(1))), dtype=np.uint64))


def parse(image):
    """-> dict(header=, entries=, accum=, sections=, data=[nlev, extent] array per section).  Checks the structure, not the
    checksums."""
    img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)
    if img.size < HEADER.itemsize:
        raise RestartError("truncated image")
    h = np.frombuffer(img[:HEADER.itemsize].tobytes(), HEADER)[0]
    if bytes(h["magic"]).ljust(8, b"\0") == MAGIC and int(h["version"]) == VERSION_RESERVOIR:
        raise RestartError("not a restart image of a format version this module reads: version 7 holds the routing state of a context "
                           "with reservoirs, cell data that is neither merged nor sliced")
    if bytes(h["magic"]).ljust(8, b"\0") != MAGIC or not VERSION <= int(h["version"]) <= MAX_VERSION:
        raise RestartError("not a restart image of this format version")
    hb, tb, ne, ns = int(h["header_bytes"]), int(h["total_bytes"]), int(h["nentries"]), int(h["nsections"])
    o = HEADER.itemsize
    na = 0
    if int(h["version"]) >= VERSION_ACCUM:
        if img.size < o + 8:
            raise RestartError("truncated image")
        na, zero = (int(x) for x in np.frombuffer(img[o:o + 8].tobytes(), "<u4"))
        if zero != 0:
            raise RestartError("the word after the accumulator count is not 0")
        o += 8
    ncalls = None
    if int(h["version"]) >= VERSION_ROUTING:
        if img.size < o + 8:
            raise RestartError("truncated image")
        ncalls = int(np.frombuffer(img[o:o + 8].tobytes(), "<i8")[0])
        if ncalls < 0:
            raise RestartError("the routing's call count is negative")
        o += 8
    if hb > img.size or tb > img.size or hb < o + ne * ENTRY.itemsize + na * ACCUM.itemsize + ns * SECTION.itemsize:
        raise RestartError("truncated image")
    ent = np.frombuffer(img[o:o + ne * ENTRY.itemsize].tobytes(), ENTRY).copy()
    o += ne * ENTRY.itemsize
    acc = np.frombuffer(img[o:o + na * ACCUM.itemsize].tobytes(), ACCUM).copy()
    o += na * ACCUM.itemsize
    sec = np.frombuffer(img[o:o + ns * SECTION.itemsize].tobytes(), SECTION).copy()
    if _version(sec, na) != int(h["version"]):
        raise RestartError(f"a version-{int(h['version'])} image with the optional sections of version {_version(sec, na)}")
    data = []
    for s in sec:
        dt = ELEM[int(s["dtype"])]
        n = int(s["nlev"]) * int(s["extent"])
        off = int(s["offset"])
        if off + n * dt.itemsize > tb:
            raise RestartError("truncated image")
        data.append(np.frombuffer(img[off:off + n * dt.itemsize].tobytes(), dt).reshape(int(s["nlev"]), int(s["extent"])))
    return dict(header=h, entries=ent, accum=acc, sections=sec, data=data, routing_ncalls=ncalls)


def verify(image):
    """parse() and check the header checksum and every section checksum; raises RestartError."""
    img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)
    p = parse(img)
    h = p["header"]
    if header_checksum(img, int(h["header_bytes"])) != int(h["header_checksum"]):
        raise RestartError("header checksum mismatch")
    for s, d in zip(p["sections"], p["data"]):
        g0 = 0 if int(s["kind"]) in CELL_SECTIONS else int(h["gcol0"])
        if checksum(d, g0) != int(s["checksum"]):
            raise RestartError(f"section checksum mismatch (kind {int(s['kind'])}, id {int(s['id'])})")
    return p


def build(header, entries, sections, data, accum=None, routing_ncalls=0):
    """An image from its parts: offsets, header_bytes, total_bytes, the version (OPTIONAL: by its sections and `accum`) and the
    header checksum are computed; section checksums are taken from sections['checksum']."""
    h = np.array(header, HEADER).reshape(())
    ent = np.asarray(entries, ENTRY)
    acc = np.zeros(0, ACCUM) if accum is None else np.asarray(accum, ACCUM).reshape(-1)
    sec = np.array(sections, SECTION)
    h["version"] = _version(sec, acc.size)
    word = int(h["version"]) >= VERSION_ACCUM  # (the count word)
    calls = int(h["version"]) >= VERSION_ROUTING  # (the routing's call count)
    pre = HEADER.itemsize + (8 if word else 0) + (8 if calls else 0)
    hb = _align(pre + ent.size * ENTRY.itemsize + acc.size * ACCUM.itemsize + sec.size * SECTION.itemsize)
    off = hb
    for i, d in enumerate(data):
        sec[i]["offset"] = off
        off = _align(off + d.nbytes)
    h["nentries"], h["nsections"], h["header_bytes"], h["total_bytes"], h["header_checksum"] = ent.size, sec.size, hb, off, 0
    img = np.zeros(off, np.uint8)
    img[:HEADER.itemsize] = np.frombuffer(h.tobytes(), np.uint8)
    if word:
        img[HEADER.itemsize:HEADER.itemsize + 8] = np.frombuffer(np.array([acc.size, 0], "<u4").tobytes(), np.uint8)
    if calls:
        img[pre - 8:pre] = np.frombuffer(np.array([routing_ncalls], "<i8").tobytes(), np.uint8)
    o = pre
    img[o:o + ent.nbytes] = np.frombuffer(ent.tobytes(), np.uint8)
    o += ent.nbytes
    img[o:o + acc.nbytes] = np.frombuffer(acc.tobytes(), np.uint8)
    o += acc.nbytes
    img[o:o + sec.nbytes] = np.frombuffer(sec.tobytes(), np.uint8)
    for s, d in zip(sec, data):
        b = np.frombuffer(np.ascontiguousarray(d, ELEM[int(s["dtype"])]).tobytes(), np.uint8)
        img[int(s["offset"]):int(s["offset"]) + b.size] = b
    img[_CK_OFF:_CK_OFF + 8] = np.frombuffer(np.uint64(header_checksum(img, hb)).tobytes(), np.uint8)
    return img


def _no_gridded(p, what):
    if np.any(np.isin(p["sections"]["kind"], (ROUTING_SECTION, IRRSUP_SECTION))):
        raise RestartError(f"{what}: a version-{VERSION_ROUTING} image holds the routing state; cell data does not follow a column decomposition")
    if np.any(p["entries"]["gridded"] == CELL_ROW_ENTRY):
        raise RestartError(f"{what}: the image holds cell-row history entries; cell data does not follow a column decomposition")
    if np.any(p["entries"]["gridded"] != 0):
        raise RestartError(f"{what}: the image holds gridded history entries, which do not survive a change of decomposition")


def merge(images):
    """Images of adjacent column ranges (any order) -> one image of their union.  Section checksums add."""
    ps = sorted((verify(i) for i in images), key=lambda p: int(p["header"]["gcol0"]))
    if not ps:
        raise RestartError("merge: no images")
    first = ps[0]
    for p in ps:
        _no_gridded(p, "merge")
    end = int(first["header"]["gcol0"])
    for p in ps:
        h = p["header"]
        if int(h["gcol0"]) != end:
            raise RestartError("merge: the column ranges are not adjacent")
        end += int(h["ncols"])
        for k in ("version", "schema_hash", "real_bytes", "nentries", "nsections"):
            if h[k] != first["header"][k]:
                raise RestartError(f"merge: the images differ in {k}")
        if not np.array_equal(h["tape_count"], first["header"]["tape_count"]) or p["entries"].tobytes() != first["entries"].tobytes():
            raise RestartError("merge: the images hold different history tapes")
        if p["accum"].tobytes() != first["accum"].tobytes():
            raise RestartError("merge: the images hold different accumulator entries or step counts")
        a, b = p["sections"], first["sections"]
        if not all(np.array_equal(a[k], b[k]) for k in ("kind", "id", "nlev", "dtype")):
            raise RestartError("merge: the images hold different sections")
    h = first["header"].copy()
    h["ncols"] = end - int(first["header"]["gcol0"])
    sec = first["sections"].copy()
    data = []
    for i in range(sec.size):
        data.append(np.concatenate([p["data"][i] for p in ps], axis=1))
        sec[i]["extent"] = h["ncols"]
        sec[i]["checksum"] = int(np.sum(np.array([int(p["sections"][i]["checksum"]) for p in ps], np.uint64), dtype=np.uint64))
    return build(h, first["entries"], sec, data, first["accum"])


def slice(image, gcol0, n):  # noqa: A001 - the name of the operation
    """Global columns [gcol0, gcol0 + n) of an image, as an image of its own; checksums recomputed."""
    p = verify(image)
    _no_gridded(p, "slice")
    h = p["header"].copy()
    lo = int(gcol0) - int(h["gcol0"])
    if lo < 0 or n < 0 or lo + n > int(h["ncols"]):
        raise RestartError("slice: the columns are outside the image")
    h["gcol0"], h["ncols"] = gcol0, n
    sec = p["sections"].copy()
    data = []
    for i in range(sec.size):
        d = np.ascontiguousarray(p["data"][i][:, lo:lo + n])
        data.append(d)
        sec[i]["extent"] = n
        sec[i]["checksum"] = checksum(d, gcol0)
    return build(h, p["entries"], sec, data, p["accum"])


def write(path, image):
    np.ascontiguousarray(image, dtype=np.uint8).tofile(path)


def read(path):
    """The image in a file, verified."""
    img = np.fromfile(path, dtype=np.uint8)
    verify(img)
    return img


def field_sections(image):
    """{field id: [nlev, ncols] array} of an image's field sections."""
    p = parse(image)
    return {int(s["id"]): d for s, d in zip(p["sections"], p["data"]) if int(s["kind"]) == FIELD}
