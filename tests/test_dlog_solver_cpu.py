"""The bounded discrete-log solver (eg_dlog_solver_*, csrc/dlog_kernels.cuh, csrc/dlog_host.hpp) without a GPU.

* tests/hostcheck/dlogcheck.cpp: the baby build and the giant walk run as lanes on the host, -DEG_BOUNDCHECK under UBSan, with 4-bit tags
  and baby tables of 2^4 and 2^6 entries (false candidates are certain; the limb classes are asserted over whole runs).
* tests/hostcheck/dlograngecheck.cpp: the pure-host range arithmetic under ASan + UBSan at the corners of the 64-bit range.
Both are stand-alone programs: a finding is a non-zero exit code.
* The six entry points are declared, exported and bound; the Python and C++ mirrors exist."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent / "hostcheck"
ROOT = HERE.parent.parent
CSRC = ROOT / "elastic_elgamal_amd" / "csrc"
P = 2**255 - 19
D = -121665 * pow(121666, P - 2, P) % P
NAMES = ["eg_dlog_solver_create", "eg_dlog_solver_destroy", "eg_dlog_solver_solve", "eg_dlog_solver_max_span", "eg_dlog_solver_table_bytes"]


def _build(exe: Path, src: Path, flags, deps):
    if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in [src, *deps]):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *flags, "-o", str(exe), str(src)])
    return exe


@pytest.fixture(scope="module")
def lane_report():
    """One run of the lane check; the tests below read its report."""
    exe = _build(HERE / "dlogcheck", HERE / "dlogcheck.cpp", ["-DEG_BOUNDCHECK", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"],
                 list(CSRC.glob("*.cuh")) + [CSRC / "dlog_host.hpp"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r.stdout


def test_lanes_find_every_value_and_nothing_else(lane_report):
    """Every m of [lo, hi) for lo in {0, 1, 37} and spans up to 600, several runs per element, the top of the 64-bit range; lo - 1, hi,
    hi + 1, -[m]G and a point with no small logarithm are not found (asserted inside the program); the class assertions of the
    bound-check build held on every path that ran."""
    assert lane_report.strip().endswith("PASS")
    m = re.search(r"lanes (\d+) found (\d+) false_candidates (\d+)", lane_report)
    lanes, found, false_candidates = map(int, m.groups())
    assert lanes > 5000 and found > 5000


def test_false_tag_hits_occur_and_lose_nothing(lane_report):
    """With 4-bit tags most candidates are false; the program confirms each against the element and found every value all the same."""
    false_candidates = int(re.search(r"false_candidates (\d+)", lane_report).group(1))
    assert false_candidates >= 1
    assert lane_report.strip().endswith("PASS")


def _edwards_add(a, b):
    (x1, y1), (x2, y2) = a, b
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + k, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - k, P - 2, P) % P)


def test_keys_are_the_affine_y_of_the_multiples_of_4B(lane_report):
    """The key of baby entry i is taken from y([4 i]B): compared with Edwards arithmetic in Python integers."""
    by = 4 * pow(5, P - 2, P) % P
    bx = 15112221349535400772501151409588531511454012693041857206046113283949847762202
    assert (-bx * bx + by * by - 1 - D * bx * bx * by * by) % P == 0
    b2 = _edwards_add((bx, by), (bx, by))
    b4 = _edwards_add(b2, b2)
    keys = {int(i): int(h, 16) for i, h in re.findall(r"^KEY (\d+) ([0-9a-f]{64})$", lane_report, re.M)}
    assert sorted(keys) == list(range(64))
    pt = (0, 1)
    for i in range(64):
        assert keys[i] == pt[1], i
        pt = _edwards_add(pt, b4)


def test_range_arithmetic_at_the_corners():
    """lo = hi, span 1, hi = 2^64 - 1, lo = 2^64 - 2, a span equal to max_span and one above it, n = 0, and the cutting of a call
    into launches: ASan + UBSan build of the pure-host header."""
    exe = _build(HERE / "dlograngecheck", HERE / "dlograngecheck.cpp", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                 [CSRC / "dlog_host.hpp"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout[-2000:] + r.stderr[-6000:]


def test_symbols_are_declared_exported_and_bound():
    import elastic_elgamal_amd as eg

    hdr = (ROOT / "include" / "eg_hip.h").read_text()
    assert "typedef struct eg_dlog_solver eg_dlog_solver;" in hdr
    lib = C.CDLL(str(eg.library_path()))
    declared = eg.exported_symbols()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in declared and hasattr(lib, n), n
    bound = eg._load()
    assert bound.eg_dlog_solver_max_span.restype is C.c_uint64 and bound.eg_dlog_solver_table_bytes.restype is C.c_size_t
    assert len(bound.eg_dlog_solver_solve.argtypes) == 7 and len(bound.eg_dlog_solver_create.argtypes) == 3
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", hdr).group(1)) == 7 == eg.ABI_VERSION == bound.eg_abi_version()
    # without a solver the two sizes are 0, and a null solver or context is refused, not dereferenced (no GPU needed)
    assert bound.eg_dlog_solver_max_span(None, 5) == 0 and bound.eg_dlog_solver_table_bytes(None) == 0
    out = C.c_void_p()
    assert bound.eg_dlog_solver_create(None, 0, C.byref(out)) == -3
    assert bound.eg_dlog_solver_solve(None, 0, None, 0, 0, None, None) == -3
    bound.eg_dlog_solver_destroy(None)


def test_mirrors_exist_and_the_cpp_header_compiles(tmp_path):
    from elastic_elgamal_amd import tally

    for name in ("solve", "max_span", "close"):
        assert callable(getattr(tally.DiscreteLogSolver, name))
    assert callable(tally.decrypt_totals) and callable(tally.decrypt_total) and callable(tally.DiscreteLogTable.get)
    src = tmp_path / "solver.cpp"
    src.write_text('#include "elastic_elgamal_hip.hpp"\n'
                   "using namespace elastic_elgamal_hip;\n"
                   "std::vector<std::optional<uint64_t>> totals(const Context& ctx, const std::vector<Element>& e) {\n"
                   "  DiscreteLogSolver s(ctx);\n"
                   "  return s.max_span(e.size()) && s.table_bytes() ? s.solve(e, 0, 1ull << 40) : std::vector<std::optional<uint64_t>>();\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
