"""The select census of the soil hydrology's host restatement (elmkernels_amd/hydrology.py).

Every `_min` / `_max` of `column()` (its nested functions included) and of `_sy` is a select on the device (dmin / dmax).  `recording()`
replaces the two functions of the module with versions that note, per call site, which operand was returned and whether an operand was
not finite; `static_sites()` counts the same call sites in the source with `ast`.  A site is (line, function, ordinal): the ordinal
orders the calls of one function on one line by their bytecode offset, that is in the order they are evaluated (an inner call before
the call that takes its result)."""
import ast
import contextlib
import inspect
import math
import sys

from elmkernels_amd import hydrology as hy

FUNCTIONS = ("column", "_sy")


class Census:
    """sites[(co_name, f_lineno, f_lasti)] = [fn, times the first operand was returned, times the second, calls with a non-finite
    operand, times the first and times the second operand was returned with both operands finite]."""

    def __init__(self):
        self.sites = {}

    def note(self, fn, key, second, nonfinite):
        s = self.sites.get(key)
        if s is None:
            s = self.sites[key] = [fn, 0, 0, 0, 0, 0]
        s[2 if second else 1] += 1
        if nonfinite:
            s[3] += 1
        else:
            s[5 if second else 4] += 1

    def by_site(self):
        """{(line, fn, ordinal): (first, second, nonfinite, first among finite operands, second among finite operands)} of the sites
        seen."""
        groups = {}
        for (_, line, lasti), (fn, *counts) in self.sites.items():
            groups.setdefault((line, fn), []).append((lasti, *counts))
        out = {}
        for (line, fn), calls in groups.items():
            for k, (_, *counts) in enumerate(sorted(calls)):
                out[(line, fn, k)] = tuple(counts)
        return out

    def one_sided(self, finite=False):
        """The sites that only ever returned the same operand; finite: counting only the calls whose operands were both finite."""
        i = 3 if finite else 0
        return sorted(s for s, v in self.by_site().items() if v[i] == 0 or v[i + 1] == 0)

    def report(self):
        sites = self.by_site()
        lines = [f"{len(sites)} sites, {len(self.one_sided())} one-sided, {sum(1 for v in sites.values() if v[2])} reached by a non-finite operand"]
        for (line, fn, k), (a, b, nf, af, bf) in sorted(sites.items()):
            mark = "   ONE-SIDED" if a == 0 or b == 0 else ("   one-sided on finite operands" if af == 0 or bf == 0 else "")
            lines.append(f"  line {line:3d} {fn}#{k}: first {a:7d}  second {b:7d}  non-finite {nf:6d}{mark}")
        return "\n".join(lines)


def _finite(x):
    return isinstance(x, int) or math.isfinite(x)


@contextlib.contextmanager
def recording(census=None):
    """Install the recording `_min` / `_max` into elmkernels_amd.hydrology; the originals come back on exit.  Yields the Census."""
    census = Census() if census is None else census
    names = {f.__code__.co_name for f in (hy.column, hy._sy)} | {"remove", "qsat", "v"}
    orig_min, orig_max = hy._min, hy._max

    def rec_min(a, b):
        f = sys._getframe(1)
        second = b < a
        if f.f_code.co_name in names and f.f_code.co_filename == _FILE:
            census.note("_min", (f.f_code.co_name, f.f_lineno, f.f_lasti), second, not (_finite(a) and _finite(b)))
        return b if second else a

    def rec_max(a, b):
        f = sys._getframe(1)
        second = a < b
        if f.f_code.co_name in names and f.f_code.co_filename == _FILE:
            census.note("_max", (f.f_code.co_name, f.f_lineno, f.f_lasti), second, not (_finite(a) and _finite(b)))
        return b if second else a

    hy._min, hy._max = rec_min, rec_max
    try:
        yield census
    finally:
        hy._min, hy._max = orig_min, orig_max


_FILE = hy.column.__code__.co_filename


def _source():
    return inspect.getsource(hy)


def static_sites():
    """{(line, fn): the number of `fn(...)` Call nodes on that line} over column() with its nested functions and over _sy."""
    tree = ast.parse(_source())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in FUNCTIONS:
            for call in ast.walk(node):
                if isinstance(call, ast.Call) and isinstance(call.func, ast.Name) and call.func.id in ("_min", "_max"):
                    key = (call.lineno, call.func.id)
                    out[key] = out.get(key, 0) + 1
    return out


def line_of(fragment):
    """The line of hydrology.py inside column() / _sy that holds `fragment` (exactly one must): the exemptions of the census name their
    sites by the text of the statement, which survives edits above it."""
    tree = ast.parse(_source())
    spans = [(n.lineno, n.end_lineno) for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCTIONS]
    found = [i + 1 for i, text in enumerate(_source().splitlines()) if fragment in text and any(a <= i + 1 <= b for a, b in spans)]
    assert len(found) == 1, (fragment, found)
    return found[0]
