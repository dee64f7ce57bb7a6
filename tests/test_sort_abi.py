"""CPU-side checks of the Sort entry points of the C ABI: hy_sort_key has the C layout in the ctypes mirror, and both entry points are bound."""
import ctypes as C
import os
import subprocess

from hyrise_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sort_key_has_the_c_layout(tmp_path):
    fields = [name for name, _ in abi.SortKey._fields_]
    assert fields == ["column", "mode", "reserved"]
    source = tmp_path / "sort_key.c"
    lines = ['  printf("size %zu\\n", sizeof(hy_sort_key));\n'] + [f'  printf("{f} %zu\\n", offsetof(hy_sort_key, {f}));\n' for f in fields]
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hyrise_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    binary = tmp_path / "sort_key"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(binary), str(source)])
    sizes = dict(line.split() for line in subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(sizes["size"]) == C.sizeof(abi.SortKey) == 16
    for f in fields:
        assert int(sizes[f]) == getattr(abi.SortKey, f).offset, f


def test_sort_entry_points_are_exported_and_bound():
    lib = abi.load_library()
    bound = {name for name, _, _ in abi.SYMBOLS}
    for name in ("hy_sort", "hy_column_gather"):
        assert name in bound and hasattr(lib, name), name
