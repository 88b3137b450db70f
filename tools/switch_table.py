"""The rows of DESIGN.md's switch table for the native library's switches, from the library's own list:
   python tools/switch_table.py      (paste over the rows between HELFEM_SCF and HELFEM_HDF5_LIB)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helfem_amd as hf  # noqa: E402

for r in hf.tuning_table():
    print("| `%s` | %s | %s | %s | %s |" % (r["name"], r["kind"], "`%s`" % r["default"] if r["default"] else "unset", r["read"], r["meaning"]))
