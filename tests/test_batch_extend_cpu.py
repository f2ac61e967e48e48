"""pcabo_batch_gp_extend / pcabo_batch_gp_truncate / pcabo_batch_gp_extended without a GPU: the surface (library, header, binding)
and the record-keeping of csrc/model_state.h, driven by the stand-alone program csrc/batch_extend_selftest.cpp, which this test
compiles with the host compiler - plain, and where the compiler has the runtimes as an address + undefined-behaviour sanitizer
build of its own (a program with its own main: nothing is loaded into Python).  The device side is tests/test_gpu_batch_extend.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "para-ortho-pca-bo_amd", "csrc")
NAMES = ("pcabo_batch_gp_extend", "pcabo_batch_gp_truncate", "pcabo_batch_gp_extended")


def test_surface(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    lib = ctypes.CDLL(native.lib_path())
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in native.EXPORTS
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2                          # additive: the version stays
    L = native.LIB
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [6, 3, 3]
    assert all(getattr(L, name).restype is ctypes.c_int for name in NAMES)
    assert callable(native.Batch.gp_extend) and callable(native.Batch.gp_truncate) and isinstance(native.Batch.n_base, property)
    # no batch: refused before any device is touched
    assert L.pcabo_batch_gp_extend(None, None, None, 1, 0, None) == -1
    assert L.pcabo_batch_gp_truncate(None, 0, None) == -1 and L.pcabo_batch_gp_extended(None, None, None) == -1


def test_the_header_documents_the_calls():
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    doc = header[header.index("pcabo_gp_extend / pcabo_gp_truncate / pcabo_gp_extended for the runs of a batch"):]
    doc = doc[: doc.index("int pcabo_batch_gp_extended(")]
    for word in ("SET ASIDE", "PCABO_ERR_NOT_PD", "PCABO_EXTEND_BELIEVER", "pcabo_batch_set_active", "n_base", "p*max_d"):
        assert word in doc, word
    assert "the lock-step batches have no such call yet" not in header
    single = header[header.index("Append p >= 1 points"): header.index("int pcabo_gp_extend(")]
    assert "pcabo_batch_gp_extend" in single                                                  # the member-context refusal points here


def _build_and_run(tmp_path, tag, flags):
    exe = str(tmp_path / ("batch_extend_selftest_" + tag))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags,
           os.path.join(CSRC, "batch_extend_selftest.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return built, (subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) if built.returncode == 0 else None)


def test_the_state_transitions_in_a_program_of_their_own(tmp_path):
    built, ran = _build_and_run(tmp_path, "plain", [])
    assert built.returncode == 0, built.stdout
    assert ran.returncode == 0 and "batch extend state: ok" in ran.stdout, ran.stdout
    # the same under AddressSanitizer + UBSan where this compiler can link them (a stand-alone build; optional)
    built, ran = _build_and_run(tmp_path, "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if built.returncode == 0:
        assert ran.returncode == 0 and "batch extend state: ok" in ran.stdout, ran.stdout
