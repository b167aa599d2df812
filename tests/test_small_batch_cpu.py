"""CPU-side checks of the small-batch entries (eg_verify_*_small[_device]): declared, exported and bound; mirrored in Python and C++;
EG_SMALL_BATCH_MAX agrees between header and binding; the ABI version and the plans of every existing kind are unchanged; without a GPU
the entries fail loudly, like the batch ones."""
import ctypes as C
import json
import re
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

import elastic_elgamal_amd as eg

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("eg_verify_choice_small", "eg_verify_choice_small_device", "eg_verify_qv_small", "eg_verify_qv_small_device")


def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    raw = C.CDLL(str(eg.library_path()))
    lib = eg._load()
    for name in SYMBOLS:
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in eg.exported_symbols()
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 5, name
    # beside the batch entries, with their arguments
    for kind, params in (("choice", "eg_choice_params"), ("qv", "eg_qv_params")):
        batch = re.search(rf"int eg_verify_{kind}_batch\(([^)]*)\)", header).group(1)
        small = re.search(rf"int eg_verify_{kind}_small\(([^)]*)\)", header).group(1)
        assert batch == small and batch.startswith(params)
        batch_d = re.search(rf"int eg_verify_{kind}_batch_device\(([^)]*)\)", header).group(1)
        small_d = re.search(rf"int eg_verify_{kind}_small_device\(([^)]*)\)", header).group(1)
        assert batch_d == small_d


def test_small_batch_max_and_abi_version():
    header = (ROOT / "include" / "eg_hip.h").read_text()
    assert int(re.search(r"#define EG_SMALL_BATCH_MAX (\d+)", header).group(1)) == eg.SMALL_BATCH_MAX == 4096
    assert int(re.search(r"#define EG_ABI_VERSION (\d+)", header).group(1)) == eg.ABI_VERSION == 7
    assert eg._load().eg_abi_version() == 7


def test_python_and_cpp_mirrors_exist(tmp_path):
    for cls in (eg.ChoiceParams, eg.QuadraticVotingParams):
        assert callable(cls.verify_small) and callable(cls.verify_small_device)
    hpp = (ROOT / "include" / "elastic_elgamal_hip.hpp").read_text()
    assert hpp.count(" verify_small(const Bytes& packed) const") == 2 and hpp.count("void verify_small_device(") == 2
    src = tmp_path / "mirror.cpp"
    src.write_text(textwrap.dedent("""
        #include "elastic_elgamal_hip.hpp"
        using namespace elastic_elgamal;
        template <class P> auto small_host(const P& p, const Bytes& b) { return p.verify_small(b); }
        template <class P> void small_dev(const P& p, const void* d, void* s) { p.verify_small_device(1, d, s); p.verify_small_device(1, d, s, nullptr); }
        int main(int argc, char**) {
          if (argc > 100) {        // instantiated, never run: there is no GPU here
            Context ctx(0);
            Element pk{};
            ChoiceParams c = ChoiceParams::single(ctx, pk, 5);
            QuadraticVotingParams q(ctx, pk, 5, 20);
            small_host(c, Bytes()); small_host(q, Bytes());
            small_dev(c, nullptr, nullptr); small_dev(q, nullptr, nullptr);
          }
          static_assert(EG_SMALL_BATCH_MAX == 4096, "header constant");
          return 0;
        }
        """))
    ns = re.search(r"^namespace (\w+)", hpp, re.M).group(1)
    src.write_text(src.read_text().replace("elastic_elgamal;", ns + ";"))
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src),
                           f"-L{ROOT / 'elastic_elgamal_amd'}", "-leg_hip", f"-Wl,-rpath,{ROOT / 'elastic_elgamal_amd'}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_header_stays_plain_c(tmp_path):
    src = tmp_path / "c_check.c"
    src.write_text('#include "eg_hip.h"\nint main(void) { return EG_SMALL_BATCH_MAX == 4096 && eg_verify_choice_small && eg_verify_qv_small_device ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_and_oversized_calls_are_refused_without_a_gpu():
    """argument checks come before any device work: a null params object or a null buffer is EG_ERR_BAD_ARG with a message, and a call
    with more than EG_SMALL_BATCH_MAX ballots is refused as such whatever else it carries; n = EG_SMALL_BATCH_MAX is not over the limit"""
    lib = eg._load()
    st = (C.c_uint32 * 1)()
    bad_arg = eg.ERR_BAD_ARG if hasattr(eg, "ERR_BAD_ARG") else int(re.search(r"EG_ERR_BAD_ARG\s*=\s*(-?\d+)", (ROOT / "include" / "eg_hip.h").read_text()).group(1))
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert fn(None, 1, None, st, None) == bad_arg, name
        assert b"EG_SMALL_BATCH_MAX" not in lib.eg_last_error() and lib.eg_last_error(), name
        assert fn(None, eg.SMALL_BATCH_MAX, None, st, None) == bad_arg, name
        assert b"EG_SMALL_BATCH_MAX" not in lib.eg_last_error(), name
        for n in (eg.SMALL_BATCH_MAX + 1, 1 << 40):
            assert fn(None, n, None, st, None) == bad_arg, (name, n)
            assert b"EG_SMALL_BATCH_MAX" in lib.eg_last_error(), (name, n)


def test_missing_gpu_is_loud():
    """without a GPU there is no context and so no params object; the Python methods have nothing behind them but the C entry, which
    refuses a call without an object: an EgError, never a quiet result"""
    import torch

    if not torch.cuda.is_available():
        with pytest.raises(eg.EgError):
            eg.Context(0)
    for cls, prefix in ((eg.ChoiceParams, "choice"), (eg.QuadraticVotingParams, "qv")):
        p = object.__new__(cls)              # what a caller would hold if a params object could exist without a GPU: no handle
        p._h, p._prefix, p.ballot_size, p.n_options = None, prefix, 736, 5
        with pytest.raises(eg.EgError, match="bad argument"):
            p.verify_small(bytes(736))
        with pytest.raises(eg.EgError, match="bad argument"):
            p.verify_small_device(1, 0, 0)
        with pytest.raises(eg.EgError, match="EG_SMALL_BATCH_MAX"):
            p.verify_small_device(eg.SMALL_BATCH_MAX + 1, 0, 0)


def test_plans_of_every_existing_kind_are_unchanged():
    before = json.loads((ROOT / "tests" / "golden" / "plan_describe_before_provers.json").read_text())
    assert {c[0] for c in before} == {"single", "multi", "qv", "zero", "bool", "range", "sumsq", "commit_equiv"}
    for kind, n, c, want in before:
        assert eg.plan_describe(kind, n, c) == want, (kind, n, c)


def test_no_new_environment_knob():
    src = (ROOT / "elastic_elgamal_amd" / "csrc" / "eg_hip.hip").read_text()
    a, b = src.index("static Knobs read_knobs()"), src.index("// Fault points:")
    assert len(set(re.findall(r'"(EG_[A-Z_]+)"', src[a:b]))) == 16
    for f in ("latency_kernels.cuh", "ge25519_quad.cuh"):
        assert "getenv" not in (ROOT / "elastic_elgamal_amd" / "csrc" / f).read_text()
