"""hy_projection_expression at the C boundary, without a GPU: the ctypes mirrors of its structs against the header, the limits, the symbol,
and the argument errors that are decided before any device work."""
import ctypes as C
import os
import re
import subprocess

from hyrise_amd import abi
from hyrise_amd.operators import projection_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hyrise_amd.h")


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"hy_projection_node": abi.ProjectionNode, "hy_projection_test": abi.ProjectionTest, "hy_projection_program": abi.ProjectionProgram, "hy_in_list": abi.InList}
    lines = [f'  printf("{name} %zu\\n", sizeof({name}));\n' for name in structs]
    for name, mirror in structs.items():
        lines += [f'  printf("{name}.{field[0]} %zu\\n", offsetof({name}, {field[0]}));\n' for field in mirror._fields_]
    source = tmp_path / "sizes.c"
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hyrise_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    binary = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(binary), str(source)])
    sizes = dict(line.split() for line in subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    for name, mirror in structs.items():
        assert int(sizes[name]) == C.sizeof(mirror), name
        for field in mirror._fields_:
            assert int(sizes[f"{name}.{field[0]}"]) == getattr(mirror, field[0]).offset, f"{name}.{field[0]}"


def test_limits_and_kinds_are_the_header_s():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    defines = {name: int(value) for name, value in re.findall(r"#define HY_MAX_PROJECTION_([A-Z]+) (\d+)", text)}
    assert defines == {"NODES": abi.MAX_PROJECTION_NODES, "DEPTH": abi.MAX_PROJECTION_DEPTH, "COLUMNS": abi.MAX_PROJECTION_COLUMNS, "TESTS": abi.MAX_PROJECTION_TESTS}
    assert abi.MAX_PROJECTION_NODES == 32 and abi.MAX_PROJECTION_DEPTH >= 4
    header = {name: int(value) for name, value in re.findall(r"\bHY_PROJ_([A-Z_]+)\s*=\s*(\d+)", text)}
    mirror = {name[5:]: value for name, value in vars(abi).items() if name.startswith("PROJ_")}
    assert header == mirror and sorted(header.values()) == list(range(17))


def test_symbol_is_exported():
    lib = abi.load_library()
    assert hasattr(lib, "hy_projection_expression")
    assert any(name == "hy_projection_expression" for name, _, _ in abi.SYMBOLS)


def call(program):
    lib = abi.load_library()
    out = C.c_void_p(0xDEAD)
    status = lib.hy_projection_expression(C.byref(program) if program is not None else None, C.byref(out))
    return status, out.value, lib.hy_last_error().decode()


def test_argument_errors_decided_on_the_host():
    lib = abi.load_library()
    assert lib.hy_projection_expression(None, None) == abi.ERR_INVALID
    status, out, _ = call(None)
    assert status == abi.ERR_INVALID
    program, _ = projection_program((abi.TYPE_INT, 1))
    assert lib.hy_projection_expression(C.byref(program), None) == abi.ERR_INVALID
    # a program without any column: what hy_projection_arithmetic answers for two literals
    status, out, message = call(projection_program(("arith", abi.ARITH_ADD, (abi.TYPE_INT, 1), (abi.TYPE_INT, 2)))[0])
    assert status == abi.ERR_INVALID and out is None and "column" in message
    left, right = abi.Operand(), abi.Operand()
    left.literal_type = right.literal_type = abi.TYPE_INT
    handle = C.c_void_p()
    assert lib.hy_projection_arithmetic(abi.ARITH_ADD, C.byref(left), C.byref(right), C.byref(handle)) == abi.ERR_INVALID
    # malformed: stack underflow, two values left, an empty program, an unknown kind, a column index out of range
    for tree in (("and", (abi.TYPE_INT, 1)), ("case", (abi.TYPE_INT, 1), (abi.TYPE_INT, 1))):
        status, out, message = call(projection_program(tree)[0])
        assert status == abi.ERR_INVALID and out is None and "pops" in message
    program, _ = projection_program((abi.TYPE_INT, 1))
    program.n_nodes = 2
    program.nodes[1] = program.nodes[0]
    status, out, message = call(program)
    assert status == abi.ERR_INVALID and out is None and "leaves 2 values" in message
    program.n_nodes = 0
    assert call(program)[0] == abi.ERR_INVALID
    program.n_nodes = 1
    program.nodes[0].kind = 99
    assert call(program)[0] == abi.ERR_INVALID
    program.nodes[0].kind = abi.PROJ_COLUMN
    assert call(program)[0] == abi.ERR_INVALID
    # types: both sides NULL, AND over a Double, negating NULL, a result that is a NULL literal
    for tree in (("arith", abi.ARITH_ADD, None, None), ("and", (abi.TYPE_DOUBLE, 1.0), (abi.TYPE_INT, 1)), ("neg", None), ("case", (abi.TYPE_INT, 1), None, None), None):
        status, out, _ = call(projection_program(tree)[0])
        assert status == abi.ERR_INVALID and out is None, tree


def test_refused_shapes_answer_unsupported_with_a_message():
    one = (abi.TYPE_INT, 1)
    for name in ("between", "cast", "extract", "function", "subquery", "parameter"):
        status, out, message = call(projection_program((name, one))[0])
        assert status == abi.ERR_UNSUPPORTED and out is None and message, name
    status, _, message = call(projection_program(("cmp", abi.PRED_BETWEEN_INCLUSIVE, one, one))[0])
    assert status == abi.ERR_UNSUPPORTED and "Between" in message
    program, _ = projection_program(one)
    program.nodes[0].literal_type = abi.TYPE_STRING
    assert call(program)[0] == abi.ERR_UNSUPPORTED
    # one entry over the stack depth, one node over the node limit
    deep = one
    for _ in range(abi.MAX_PROJECTION_DEPTH):
        deep = ("arith", abi.ARITH_ADD, one, deep)
    status, _, message = call(projection_program(deep)[0])
    assert status == abi.ERR_UNSUPPORTED and "stack" in message
    at_limit = one
    for _ in range(abi.MAX_PROJECTION_DEPTH - 1):
        at_limit = ("arith", abi.ARITH_ADD, one, at_limit)
    assert call(projection_program(at_limit)[0])[0] == abi.ERR_INVALID   # (fits; refused only for having no column)
    long_chain = one
    for _ in range(16):
        long_chain = ("arith", abi.ARITH_ADD, long_chain, one)
    status, _, message = call(projection_program(long_chain)[0])
    assert status == abi.ERR_UNSUPPORTED and "33 nodes" in message   # (the true count reaches the library)
