"""CPU-side checks of the product: the C-ABI library loads and exports every symbol declared in
include/eg_hip.h; the host plan builders (pure host logic) produce the reference's shapes.  No compute calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib_path():
    import elastic_elgamal_amd as eg

    p = eg.library_path()
    if not p.exists():
        eg.build()
    return p


def test_library_exports_every_declared_symbol(lib_path):
    import elastic_elgamal_amd as eg

    lib = C.CDLL(str(lib_path))
    names = eg.exported_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/eg_hip.h but not exported"


def test_no_oracle_in_product():
    # the product must not include / link / import anything under oracle/
    for f in (ROOT / "elastic_elgamal_amd").rglob("*"):
        if f.is_file() and f.suffix in {".py", ".hip", ".cuh", ".hpp", ".h", ".cpp"}:
            txt = f.read_text()
            assert not re.search(r'#include\s+"[^"]*oracle', txt), f
            assert not re.search(r"^\s*(from|import)\s+oracle", txt, re.M), f
    out = subprocess.run(["ldd", str(ROOT / "elastic_elgamal_amd" / "libeg_hip.so")], capture_output=True, text=True).stdout
    assert "liboracle" not in out


def test_no_test_hooks_and_one_documented_list_of_knobs(lib_path):
    """VERDICT r4 task 5: no failure-injection switch in the shipped product (sources, Python, binary); the environment is read in ONE
    function of the library (read_knobs) and the table "RUN-TIME KNOBS" of include/eg_hip.h lists exactly the names it reads."""
    pkg = ROOT / "elastic_elgamal_amd"
    for f in pkg.rglob("*"):
        if f.is_file() and f.suffix in {".py", ".hip", ".cuh", ".hpp", ".h", ".cpp"}:
            assert "EG_TEST" not in f.read_text(), f
    assert b"EG_TEST" not in (pkg / "libeg_hip.so").read_bytes()
    src = (pkg / "csrc" / "eg_hip.hip").read_text()
    a, b = src.index("static Knobs read_knobs()"), src.index("// Fault points:")
    assert "getenv" not in src[:a] + src[b:], "the environment is read outside read_knobs"
    for f in (pkg / "csrc").iterdir():
        if f.name != "eg_hip.hip" and f.suffix in {".hip", ".cuh", ".hpp", ".h"}:
            assert "getenv" not in f.read_text(), f
    read = set(re.findall(r'"(EG_[A-Z_]+)"', src[a:b]))
    header = (ROOT / "include" / "eg_hip.h").read_text()
    table = header[header.index("RUN-TIME KNOBS"):header.index("#ifndef EG_HIP_H")]
    listed = set(re.findall(r"^ \*   (EG_[A-Z_]+) ", table, re.M))
    assert read == listed and len(read) == 16, (read ^ listed)
    py_env = set(re.findall(r'environ(?:\.get)?[\[(]"(EG_[A-Z_]+)"', "".join(f.read_text() for f in pkg.glob("*.py"))))
    py_env |= set(re.findall(r'"(EG_[A-Z_]+)" in os\.environ', "".join(f.read_text() for f in pkg.glob("*.py"))))
    assert py_env == {"EG_LIB", "EG_NO_TORCH_PRELOAD"} and all(k in table for k in py_env), py_env


def test_header_is_plain_c(tmp_path):
    """The boundary is a C ABI: include/eg_hip.h must be valid C99 on its own (a cgo / JNI / ctypes binding includes it from C)."""
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return eg_prepared_point_size() == 96 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ballot_sizes_and_missing_gpu_is_loud(lib_path):
    import elastic_elgamal_amd as eg

    lib = eg._load()
    assert lib.eg_choice_ballot_size(5, 1) == 736      # SURVEY 8a / BASELINE.md section 4
    assert lib.eg_choice_ballot_size(16, 0) == 2080
    import torch

    if not torch.cuda.is_available():
        with pytest.raises(eg.EgError):
            eg.Context(0)   # no silent CPU fallback


def test_cpp_host_header_compiles(tmp_path, lib_path):
    # the C++ mirror of the reference interface and the voting example build against the C ABI without a GPU
    root = ROOT
    exe = tmp_path / "voting"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", f"-I{root / 'include'}", str(root / "examples" / "voting.cpp"),
                           f"-L{root / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{root / 'elastic_elgamal_amd'}",
                           "-o", str(exe)])
    assert exe.exists()


@pytest.mark.parametrize(
    "ub,text",
    [
        (5, "0..5"), (10, "2 * 0..5 + 0..2"), (16, "4 * 0..4 + 0..4"), (17, "4 * 0..4 + 0..5"), (20, "4 * 0..5 + 0..4"),
        (21, "3 * 0..7 + 0..3"), (42, "6 * 0..7 + 0..6"), (60, "12 * 0..5 + 3 * 0..4 + 0..3"),
        (100, "20 * 0..5 + 4 * 0..5 + 0..4"), (101, "20 * 0..5 + 4 * 0..5 + 0..5"),
        (1000, "125 * 0..8 + 25 * 0..5 + 5 * 0..5 + 0..5"),
        (12345, "2880 * 0..4 + 720 * 0..5 + 90 * 0..9 + 15 * 0..7 + 3 * 0..5 + 0..3"),
        (777777, "125440 * 0..6 + 25088 * 0..6 + 3136 * 0..8 + 784 * 0..4 + 196 * 0..4 + 49 * 0..5 + 7 * 0..7 + 0..7"),
        (12345678, "3072000 * 0..4 + 768000 * 0..4 + 192000 * 0..4 + 48000 * 0..5 + 9600 * 0..6 + 1200 * 0..8 + 300 * 0..4 + "
                   "75 * 0..5 + 15 * 0..5 + 3 * 0..6 + 0..3"),
    ],
)
def test_product_range_decomposition_known_answers(lib_path, ub, text):
    # the reference's known answers (range.rs:592-662 and the doc table :56-65) against the PRODUCT's host code
    import elastic_elgamal_amd as eg

    assert eg.range_decomposition(ub) == text


def test_product_range_decomposition_matches_oracle(lib_path, oracle):
    import elastic_elgamal_amd as eg

    for ub in list(range(2, 200)) + [255, 256, 257, 500, 999, 1024, 4096, 65535]:
        assert eg.range_decomposition(ub) == oracle.PreparedRange(ub).name, ub
    with pytest.raises(eg.EgError):
        eg.range_decomposition(1)


def test_plan_shapes(lib_path):
    import elastic_elgamal_amd as eg

    a = eg.plan_describe("single", 5)
    assert a["stride"] == 736 and a["wire_points"] == 10 and a["wire_scalars"] == 13
    assert a["stages"] == 2 and a["jobs_per_stage"] == [14, 10] and a["bases"] == 10
    assert a["table_terms"] == 22 and a["var_terms"] == 22 and a["rules"] == 2 and a["tally_slots"] == 10
    # the two log-equality bases (sums of the ring bases) take their comb tables from the ring bases' tables: no ladder is left
    assert a["sum_tables"] == 2 and a["sum_table_members"] == 10 and a["direct_terms"] == 0 and a["single_table_jobs"] == 22
    two = eg.plan_describe("single", 2)
    assert two["sum_tables"] == 0 and two["chains"] == 2                # two options: both terms on one doubling chain instead
    c = eg.plan_describe("multi", 16)
    assert c["stride"] == 2080 and c["wire_points"] == 32 and c["wire_scalars"] == 33 and c["jobs_per_stage"] == [32, 32]
    b = eg.plan_describe("qv", 5, 20)
    assert b["stride"] == 2144 and b["wire_points"] == 14 and b["wire_scalars"] == 53
    assert b["stages"] == 7                                            # longest ring: 0..7 of the credit range
    # 35 ring equations x 2 + 5 x 2 + 2 sum-of-squares equations + 2 encodes of the derived last credit ciphertext
    assert b["jobs"] == 70 + 12 + 2 and b["rules"] == 7
    assert eg.plan_describe("zero")["stride"] == 128 and eg.plan_describe("bool")["stride"] == 160
    assert eg.plan_describe("range", 0, 100)["stride"] == 672
    # comb shape of the per-ballot tables (host_plan.hpp: plan_teeth): 5 teeth where a table serves two products (rings of two), 6 for the
    # rings of 3 .. 7 of the range proofs
    assert a["teeth"] == 5 and c["teeth"] == 5 and eg.plan_describe("single", 150)["teeth"] == 5
    assert b["teeth"] == 6 and eg.plan_describe("qv", 5, 4)["teeth"] == 6 and eg.plan_describe("range", 0, 100)["teeth"] == 6
    assert eg.plan_describe("bool")["teeth"] in (5, 6)


def test_bench_static_sanity():
    """bench.py cannot run without a GPU; at least every global name it uses must be defined (a NameError on the GPU box
    would cost the round its measurement) and the VALU work model must reproduce the documented per-ballot counts."""
    import ast
    import builtins
    import importlib.util

    path = ROOT / "bench.py"
    tree = ast.parse(path.read_text())
    defined = set(dir(builtins)) | {"__file__", "__name__"}
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            defined.add(node.name)
            for a in node.args.args + node.args.kwonlyargs if isinstance(node, ast.FunctionDef) else []:
                defined.add(a.arg)
        elif isinstance(node, (ast.Import, ast.ImportFrom)):
            for a in node.names:
                defined.add((a.asname or a.name).split(".")[0])
        elif isinstance(node, ast.Name) and isinstance(node.ctx, (ast.Store, ast.Del)):
            defined.add(node.id)
        elif isinstance(node, ast.arg):
            defined.add(node.arg)
        elif isinstance(node, ast.ExceptHandler) and node.name:
            defined.add(node.name)
    used = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load)}
    assert not (used - defined), used - defined
    spec = importlib.util.spec_from_file_location("bench_mod", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import elastic_elgamal_amd as eg

    fm, fs = mod.plan_field_ops(eg.plan_describe("single", 5))
    assert 22_000 < fm < 35_000 and 14_000 < fs < 22_000
    qm, qs = mod.plan_field_ops(eg.plan_describe("qv", 5, 20))          # a QV ballot is 2-3x a single-choice ballot
    assert 2 * fm < qm < 4 * fm and 1.5 * fs < qs < 4 * fs
    mm, ms = mod.plan_field_ops(eg.plan_describe("multi", 16))          # 32 ring bases instead of 10, no sum proof
    assert 2.5 * fm < mm < 3.5 * fm
    assert mod.effective_cores() >= 1


def test_integration_ffi_block_matches_header():
    """INTEGRATION.md shows the binding a maintainer of the reference would write (`extern "C"` in Rust).  It must declare every
    function of include/eg_hip.h with the same number of arguments, and equal what tools/gen_ffi.py generates from the header."""
    import importlib.util
    import re

    spec = importlib.util.spec_from_file_location("gen_ffi", ROOT / "tools" / "gen_ffi.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    header = {name: len(params) for _, name, params in gen.prototypes((ROOT / "include" / "eg_hip.h").read_text())}
    assert len(header) >= 55 and "eg_verify_choice_batch_device" in header and "eg_points_sum_device" in header
    doc = (ROOT / "INTEGRATION.md").read_text()
    block = doc[doc.index(gen.BEGIN) : doc.index(gen.END)]
    declared = {}
    for m in re.finditer(r"pub fn (eg_[a-z0-9_]+)\(([^)]*)\)", block):
        args = [a for a in m.group(2).split(",") if a.strip()]
        declared[m.group(1)] = len(args)
    assert declared == header
    assert gen.rust_block() in block                      # regenerate with `python tools/gen_ffi.py --update`
    import elastic_elgamal_amd as eg

    assert set(eg.exported_symbols()) == set(header)      # the two header parsers agree


def test_gpus_are_counted_without_hip(tmp_path):
    """bench.py's bare launcher counts the GPUs from the KFD topology (VERDICT r5 task 1: torch.cuda.device_count() may initialise the
    runtime in the parent): nodes with simd_count > 0, then ROCR_VISIBLE_DEVICES and HIP_ / CUDA_VISIBLE_DEVICES as the runtimes apply them."""
    import importlib.util
    from pathlib import Path

    spec = importlib.util.spec_from_file_location("bench_for_test", Path(__file__).resolve().parent.parent / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert "torch" not in bench.__dict__                       # importing bench.py imports neither torch nor the library
    topo = tmp_path / "nodes"
    simd = [0, 0, 1024, 1024, 1024, 1024]                       # two CPU nodes, four GPUs
    for i, sc in enumerate(simd):
        (topo / str(i)).mkdir(parents=True)
        (topo / str(i) / "properties").write_text(f"cpu_cores_count {0 if sc else 64}\nsimd_count {sc}\nunique_id {1000 + i}\n")
    count = lambda **env: bench.count_gpus_without_hip(str(topo), env)
    assert count() == 4
    assert count(HIP_VISIBLE_DEVICES="0,1") == 2 and count(CUDA_VISIBLE_DEVICES="2") == 1
    assert count(HIP_VISIBLE_DEVICES="1,7,2") == 1                # the list ends at the first entry that is not a visible device
    assert count(ROCR_VISIBLE_DEVICES="0,1,2") == 3 and count(ROCR_VISIBLE_DEVICES="0,1,2", HIP_VISIBLE_DEVICES="0,2,3") == 2
    assert count(ROCR_VISIBLE_DEVICES="GPU-%x" % 1003) == 1 and count(ROCR_VISIBLE_DEVICES="GPU-deadbeef") == 0
    assert count(ROCR_VISIBLE_DEVICES="GPU-not-hex,0") == 0
    assert count(HIP_VISIBLE_DEVICES="") == 0 and count(HIP_VISIBLE_DEVICES="-1") == 0
    assert bench.count_gpus_without_hip(str(tmp_path / "absent"), {}) is None


def test_bench_options_and_output_dump(tmp_path, monkeypatch):
    """bench.py's --full is off by default, --steps below 1 is refused, and --dump-outputs writes float64 arrays that stay within the
    budget: an array too large for its share becomes a fixed, seeded sample of its rows, their indices beside it."""
    import importlib.util
    import sys

    import numpy as np

    spec = importlib.util.spec_from_file_location("bench_for_test", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.steps == 7 and args.warmup == 2 and args.full is False and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()

    status = np.arange(1000, dtype=np.uint32) * 4_000_000            # verdict words use all 32 bits
    tally = np.arange(320, dtype=np.uint64).astype(np.uint8)
    bench.dump_outputs(tmp_path / "a", {"status": status, "tally": tally})
    assert np.load(tmp_path / "a" / "status.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), status) and np.array_equal(np.load(tmp_path / "a" / "tally.npy"), tally)
    assert not (tmp_path / "a" / "status_rows.npy").exists()
    big = np.arange(300_000 * 4, dtype=np.uint32).reshape(300_000, 4)
    for d in ("b", "c"):
        bench.dump_outputs(tmp_path / d, {"big": big, "tally": tally}, budget=2_000_000)
    rows = np.load(tmp_path / "b" / "big_rows.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "c" / "big_rows.npy")) and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), big[rows]) and len(rows) > 10_000
    assert sum(f.stat().st_size for f in (tmp_path / "b").iterdir()) <= 2_000_000


def test_abi_version_and_release_counter_without_a_gpu(lib_path):
    """Two entry points that need no GPU: eg_abi_version is the header's EG_ABI_VERSION (and the Python binding's), and the ready-made
    release function of eg_verify_json_feed_owned counts into the size_t it is given (NULL: does nothing)."""
    import ctypes as C
    import re

    import elastic_elgamal_amd as eg

    lib = C.CDLL(str(lib_path))
    lib.eg_abi_version.restype = C.c_int
    hdr = (ROOT / "include" / "eg_hip.h").read_text()
    assert lib.eg_abi_version() == int(re.search(r"#define EG_ABI_VERSION (\d+)", hdr).group(1)) == eg.ABI_VERSION
    lib.eg_json_release_count.restype = None
    lib.eg_json_release_count.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    n = C.c_size_t(41)
    lib.eg_json_release_count(C.byref(n), None, 0)
    lib.eg_json_release_count(None, None, 0)
    assert n.value == 42
