#!/usr/bin/env python3
"""What ctypes holds for every export of libpcabo.so: {name: [repr(restype), [repr(t) for t in argtypes]]} as JSON (CPU only).

    python tools/cpu_abi_dump.py OUT.json            # dump this tree's declarations
    python tools/cpu_abi_dump.py A.json B.json       # compare two dumps: prints every name that differs, exit 1 if any

Run it before and after a change to pcabo/_native.py's declarations: the two dumps are equal unless a declaration moved.
hostrng and bbob_device are imported and a DeviceObjectives is attempted first (it fails without a device, after declaring), so
declarations made there, at import or lazily, are in the dump too.  A function without argtypes dumps as an empty list."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))

DEBUG = ("pcabo_debug_lbfgsb_branch_names", "pcabo_debug_lbfgsb_branches", "pcabo_debug_batch_lbfgsb_branches",
         "pcabo_debug_batch_lbfgsb_device_out")


def dump():
    from pcabo import _native, hostrng, bbob_device  # noqa: F401
    from pcabo.bbob import BBOBProblem
    try:
        bbob_device.DeviceObjectives([BBOBProblem(15, 0, 4)]).close()
    except _native.PcaboError:
        pass
    out = {}
    for name in list(_native.EXPORTS) + [n for n in DEBUG if hasattr(_native.LIB, n)]:
        fn = getattr(_native.LIB, name)
        out[name] = [repr(fn.restype), [repr(t) for t in (fn.argtypes or ())]]
    return out


def main(argv):
    if len(argv) == 1:
        with open(argv[0], "w") as f:
            json.dump(dump(), f, indent=1, sort_keys=True)
        return 0
    a, b = (json.load(open(p)) for p in argv)
    diff = sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))
    for n in diff:
        print(f"{n}:\n  {a.get(n)}\n  {b.get(n)}")
    print(f"{len(a)} and {len(b)} functions, {len(diff)} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
