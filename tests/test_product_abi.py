"""The Product entry points at the C boundary, without a device: both symbols are exported and bound, hy_product_result has the layout
abi.py gives it, and the addition left HY_ABI_VERSION where it was."""
import ctypes as C
import os
import subprocess

from hyrise_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_product_symbols_are_exported_and_bound():
    lib = abi.load_library()
    bound = {name: argtypes for name, _, argtypes in abi.SYMBOLS}
    for name in ("hy_product", "hy_product_count"):
        assert hasattr(lib, name), f"{name} not exported"
        assert name in bound and len(bound[name]) == 3
    assert lib.hy_abi_version() == 4


def test_product_result_layout_matches_the_header(tmp_path):
    fields = [name for name, _ in abi.ProductResult._fields_]
    assert fields == ["mem", "reserved", "left_pos", "right_pos", "pair_offsets", "capacity", "n_rows"]
    lines = ['  printf("size %zu\\n", sizeof(hy_product_result));\n'] + [f'  printf("{f} %zu\\n", offsetof(hy_product_result, {f}));\n' for f in fields]
    source = tmp_path / "product_sizes.c"
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hyrise_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    binary = tmp_path / "product_sizes"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(binary), str(source)])
    sizes = dict(line.split() for line in subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(sizes["size"]) == C.sizeof(abi.ProductResult) == 48
    for f in fields:
        assert int(sizes[f]) == getattr(abi.ProductResult, f).offset, f


def test_null_arguments_are_refused_before_any_device_work():
    lib = abi.load_library()
    n = C.c_uint64(7)
    assert lib.hy_product(None, None, None) == abi.ERR_INVALID
    assert lib.hy_product_count(None, None, C.byref(n)) == abi.ERR_INVALID and n.value == 0
    assert lib.hy_product_count(None, None, None) == abi.ERR_INVALID
