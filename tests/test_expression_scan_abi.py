"""hy_table_scan_expression at the C boundary, without a GPU: the symbol, the ABI version, and the argument errors that are decided on the
host -- with nothing written to the result."""
import ctypes as C

import numpy as np

from hyrise_amd import abi
from hyrise_amd.operators import HostScanResult, projection_program

ONE = (abi.TYPE_INT, 1)


def test_symbol_is_exported_and_the_abi_version_stays():
    lib = abi.load_library()
    assert hasattr(lib, "hy_table_scan_expression")
    assert any(name == "hy_table_scan_expression" for name, _, _ in abi.SYMBOLS)
    assert lib.hy_abi_version() == 4


def call(program):
    """-> (status, message); asserts that the result's arrays and total are as they were."""
    lib = abi.load_library()
    result = HostScanResult(3, 8)
    for array in (result.matches, result.offsets, result.counts, result.chunk_state):
        array[...] = 0xAB
    result.c.total_matches = 0xDEAD
    before = [array.copy() for array in (result.matches, result.offsets, result.counts, result.chunk_state)]
    status = lib.hy_table_scan_expression(C.byref(program) if program is not None else None, None, 0, C.byref(result.c))
    for was, array in zip(before, (result.matches, result.offsets, result.counts, result.chunk_state)):
        np.testing.assert_array_equal(array, was, err_msg="nothing is written on error")
    assert result.c.total_matches == 0xDEAD
    return status, lib.hy_last_error().decode()


def test_null_arguments():
    lib = abi.load_library()
    program, _ = projection_program(("cmp", abi.PRED_EQUALS, ONE, ONE))
    assert lib.hy_table_scan_expression(None, None, 0, None) == abi.ERR_INVALID
    assert lib.hy_table_scan_expression(C.byref(program), None, 0, None) == abi.ERR_INVALID
    assert call(None)[0] == abi.ERR_INVALID
    result = HostScanResult(1, 1)
    assert lib.hy_table_scan_expression(C.byref(program), None, 2, C.byref(result.c)) == abi.ERR_INVALID   # an excluded count without a list


def test_a_root_that_is_no_predicate_is_invalid():
    for tree in (ONE, ("arith", abi.ARITH_ADD, ONE, ONE), ("neg", ONE), ("case", ("cmp", abi.PRED_EQUALS, ONE, ONE), ONE, ONE)):
        status, message = call(projection_program(tree)[0])
        assert status == abi.ERR_INVALID and "PosList" in message, tree


def test_a_program_without_columns_is_invalid():
    for tree in (("cmp", abi.PRED_LESS_THAN, ONE, (abi.TYPE_DOUBLE, 2.0)), ("and", ("is_null", ONE), ("cmp", abi.PRED_EQUALS, ONE, ONE)), ("or", ONE, ONE), ("is_not_null", None)):
        status, message = call(projection_program(tree)[0])
        assert status == abi.ERR_INVALID and "column" in message, tree


def test_between_and_the_other_named_kinds_are_unsupported():
    for name in ("between", "cast", "extract", "function", "subquery", "parameter"):
        status, message = call(projection_program(("is_null", (name, ONE)))[0])
        assert status == abi.ERR_UNSUPPORTED and message, name
    status, message = call(projection_program(("cmp", abi.PRED_BETWEEN_INCLUSIVE, ONE, ONE))[0])
    assert status == abi.ERR_UNSUPPORTED and "Between" in message


def test_malformed_programs_and_results():
    lib = abi.load_library()
    status, message = call(projection_program(("and", ONE))[0])
    assert status == abi.ERR_INVALID and "pops" in message
    program, _ = projection_program(("cmp", abi.PRED_EQUALS, ONE, ONE))
    program.n_nodes = 0
    assert call(program)[0] == abi.ERR_INVALID
    program, _ = projection_program(("cmp", abi.PRED_EQUALS, ONE, ONE))
    result = HostScanResult(1, 1)
    result.c.offsets = None
    assert lib.hy_table_scan_expression(C.byref(program), None, 0, C.byref(result.c)) == abi.ERR_INVALID
    device_result = abi.ScanResult()
    device_result.mem, device_result.flags = abi.MEM_DEVICE, 0   # a device result without HY_SCAN_CHUNK_REGIONS
    device_result.offsets = 0x1000
    assert lib.hy_table_scan_expression(C.byref(program), None, 0, C.byref(device_result)) == abi.ERR_INVALID
    device_result.flags = abi.SCAN_CHUNK_REGIONS   # matches on an 8-byte boundary only: refused before anything else is looked at
    device_result.matches, device_result.capacity, device_result.counts = 0x1008, 4, 0x2000
    assert lib.hy_table_scan_expression(C.byref(program), None, 0, C.byref(device_result)) == abi.ERR_INVALID
    assert "16-byte" in lib.hy_last_error().decode()
