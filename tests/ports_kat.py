"""Prints what profiles/ports/kat.txt records: every measured value tests/test_ports_cpu.py leans on, from one run of each scene of
tests/ports_cases.py through the double-precision oracle.  python tests/ports_kat.py > profiles/ports/kat.txt"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, pkg  # noqa: E402
import ports_cases as pc  # noqa: E402

if __name__ == "__main__":
    lib = pkg("_capi").bind(ctypes.CDLL(os.path.join(ROOT, "oracle", "libfdtd_oracle_f64.so")))
    print("# python tests/ports_kat.py > profiles/ports/kat.txt")
    print("# the scenes of tests/ports_cases.py, each run once through oracle/libfdtd_oracle_f64.so; worst case over 11-17 GHz (WG, 25 points)")
    print("# and 2-10 GHz (MSL, 17 points).  tests/test_ports_cpu.py asserts at twice these values (linear); the factor covers the float32 step")
    print("# loop (budget 1.7e-5), far below PML reflection and grid dispersion, which set the values themselves.")
    for name, v in {**pc.wg_measures(lib), **pc.msl_measures(lib)}.items():
        print(f"{name} = {v:.6e}")
