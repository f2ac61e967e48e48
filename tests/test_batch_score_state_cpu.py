"""pcabo_batch_acq_score / _begin / _end without a GPU: the surface (library, header, binding) and the precondition the call adds
to csrc/model_state.h (BatchState::value_scorable and the transitions of its two halves), driven by the stand-alone program
csrc/batch_score_selftest.cpp, which this test compiles with the host compiler - plain, and where the compiler has the runtimes as
an address + undefined-behaviour sanitizer build of its own (a program with its own main: nothing is loaded into Python).  The
device side is tests/test_gpu_q_batch.py."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "para-ortho-pca-bo_amd", "csrc")
NAMES = ("pcabo_batch_acq_score", "pcabo_batch_acq_score_begin", "pcabo_batch_acq_score_end", "pcabo_bbob_eval_many")


def test_surface(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    lib = ctypes.CDLL(native.lib_path())
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in native.EXPORTS
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2                          # additive: the version stays
    L = native.LIB
    assert [len(getattr(L, name).argtypes) for name in NAMES[:3]] == [8, 6, 4]
    assert all(callable(getattr(native.Batch, name)) for name in ("acq_score", "acq_score_begin", "acq_score_end"))
    # no batch, no objective: refused before any device is touched
    assert L.pcabo_batch_acq_score(None, None, 1, None, 0, 0, None, None) == -1
    assert L.pcabo_batch_acq_score_begin(None, None, 1, None, 0, 0) == -1 and L.pcabo_batch_acq_score_end(None, 1, None, None) == -1
    from pcabo.bbob_device import DeviceObjectives
    assert callable(DeviceObjectives.eval_many)
    lib.pcabo_bbob_eval_many.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.pcabo_bbob_eval_many(None, None, 3, -5.0, 5.0, 1000.0, None, None) == -1


def test_the_header_documents_the_call():
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    doc = header[header.index("Score q points per run on the batch's model AS IT STANDS"): header.index("int pcabo_batch_acq_score_end(")]
    for word in ("values only", "extended", "PCABO_ERR_ARG", "set aside", "pcabo_batch_gp_condition_end_eval", "_begin"):
        assert word in doc, word


def _build_and_run(tmp_path, tag, flags):
    exe = str(tmp_path / ("batch_score_selftest_" + tag))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags,
           os.path.join(CSRC, "batch_score_selftest.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return built, (subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) if built.returncode == 0 else None)


def test_the_state_transitions_in_a_program_of_their_own(tmp_path):
    built, ran = _build_and_run(tmp_path, "plain", [])
    assert built.returncode == 0, built.stdout
    assert ran.returncode == 0 and "batch score state: ok" in ran.stdout, ran.stdout
    # the same under AddressSanitizer + UBSan where this compiler can link them (a stand-alone build; optional)
    built, ran = _build_and_run(tmp_path, "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if built.returncode == 0:
        assert ran.returncode == 0 and "batch score state: ok" in ran.stdout, ran.stdout
