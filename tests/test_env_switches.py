"""The documented switches are the ones the code reads.  Host-only, no library:
the FAMG_* names read in faer-amg_amd/csrc and the Python package against the
names INTEGRATION.md lists, and the flag table of include/amg.h against the
flags of csrc/common.hpp (FLAG_COUNT) and the variables capi.cpp seeds them from."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "faer-amg_amd")


def read(*parts):
    with open(os.path.join(*parts), encoding="utf-8") as f:
        return f.read()


def test_integration_md_lists_the_switches_the_code_reads():
    files = glob.glob(os.path.join(PKG, "csrc", "*")) + \
        glob.glob(os.path.join(PKG, "faer_amg_amd", "**", "*.py"), recursive=True)
    assert files
    read_by_code = set()
    for path in files:
        read_by_code.update(re.findall(r'"(FAMG_[A-Z0-9_]+)"', read(path)))
    documented = set(re.findall(r"FAMG_[A-Z0-9_]+", read(ROOT, "INTEGRATION.md")))
    assert len(read_by_code) > 40  # the scan found the sources
    assert sorted(read_by_code - documented) == [], "read but not in INTEGRATION.md"
    assert sorted(documented - read_by_code) == [], "in INTEGRATION.md but read nowhere"


def test_amg_h_documents_every_flag():
    count = int(re.search(r"FLAG_COUNT = (\d+)", read(PKG, "csrc", "common.hpp")).group(1))
    rows = re.findall(r"^ \*   flag (\d+) +(FAMG_[A-Z0-9_]+) ", read(ROOT, "include", "amg.h"), re.M)
    assert [int(i) for i, _ in rows] == list(range(count))
    # the same variables, in flag order, seed the flags
    table = re.search(r"g_flag_val\[FLAG_COUNT\] = \{(.*?)\};\n", read(PKG, "csrc", "capi.cpp"), re.S).group(1)
    assert re.findall(r'"(FAMG_[A-Z0-9_]+)"', table) == [name for _, name in rows]
