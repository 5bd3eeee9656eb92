"""CPU: the physics of the matrix-free brick operator is decided once.  tools/host_check_brick_operator_physics.cpp walks the rows of
csrc/brick_operator_physics.h (one row per tag 1 to 4, fields and order, the parameter block against the set-params entry point, the multigrid
entry point, the signed diagonal), compiled plain and as the same stand-alone program under the address and undefined-behaviour sanitizers.  The
(entry point, physics) message table of csrc/brick_multigrid.hip holds the words of the commit before it existed
(tests/golden/brick_multigrid_refusals.json: taken from that commit's source); the tag is tested nowhere but in the tables; brick_operator.hip holds
no kernel."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metafem.jl_amd", "csrc")
LITERAL = r'"((?:[^"\\]|\\.)*)"'


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _code(text):
    """without // comments (no string of these files holds two slashes)"""
    return "\n".join(line.split("//")[0] for line in text.splitlines())


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_host_check_brick_operator_physics(flags, tmp_path):
    exe = str(tmp_path / "host_check_brick_operator_physics")
    subprocess.run(["g++", *flags, "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tools", "host_check_brick_operator_physics.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("OK")
    rows = re.findall(r"^tag (\d): (.+?), (\d) field\(s\), order (\d), block (\d), set-params (\d), multigrid (-?\d), signed diagonal (\d)$", out.stdout, flags=re.M)
    assert [(int(t), int(f), int(o)) for t, _, f, o, *_ in rows] == [(1, 1, 1), (2, 3, 1), (3, 1, 2), (4, 3, 2)]
    assert [r[1] for r in rows] == ["hex-8 thermal", "hex-8 elasticity", "hex-27 thermal", "hex-27 elasticity"]


def test_the_header_is_plain_and_the_tags_are_the_enums():
    physics, shared = _read("brick_operator_physics.h"), _read("brick_operator.h")
    assert "#include" not in _code(physics) and "__device__" not in physics and "hip" not in _code(physics).lower()
    assert '#include "brick_operator_physics.h"' in shared
    assert re.search(r"enum \{ BOP_PHYSICS_THERMAL = 1, BOP_PHYSICS_ELASTICITY = 2, BOP_PHYSICS_HEX27 = 3, BOP_PHYSICS_ELASTICITY_HEX27 = 4 \}", shared)
    assert "static_assert(BOP_PHYSICS_THERMAL == 1 && BOP_PHYSICS_ELASTICITY == 2 && BOP_PHYSICS_HEX27 == 3 && BOP_PHYSICS_ELASTICITY_HEX27 == BOP_PHYSICS_ROWS" in shared
    assert re.findall(r"^\s*\{(\d), \d, \d, BOP_BLOCK_", physics, flags=re.M) == ["1", "2", "3", "4"]


def _function(text, head):
    """the body of the function whose definition starts with `head`, up to the closing brace in column 0"""
    start = text.index(head)
    return text[start:text.index("\n}\n", start)]


def test_message_table_holds_the_parents_words():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "brick_multigrid_refusals.json")))["strings"]
    assert len(golden) == 8 and len(set(golden)) == 8
    table = _function(_read("brick_multigrid.hip"), "static const char* mg_wrong_physics(int which, int tag) {")
    literals = re.findall(LITERAL, _code(table))
    assert sorted(literals) == sorted(golden)  # every string of the table is the parent's, verbatim, and none of the parent's is lost
    assert table.count("bop_e27_multigrid_refusal()") == 4  # one per entry point: the hex-27 elasticity column
    rows = re.findall(r"^\s+\{(.+?)\}[,}]", table[table.index("why[BOP_MG_ENTRIES][BOP_PHYSICS_ROWS]"):], flags=re.M)
    assert len(rows) == 4
    # the entry point that serves a physics has no message for it: create and create_nonsymmetric thermal, create_elasticity and create_hex27 their own
    served = [[cell.strip() == "nullptr" for cell in row.split(",")] for row in rows]  # (no string of the table holds a comma)
    assert served == [[True, False, False, False], [True, False, False, False], [False, True, False, False], [False, False, True, False]]
    assert "does not exist yet" in _read("brick_operator_elasticity_hex27_decide.h")


def test_the_tag_is_tested_in_the_tables_only():
    handle = _code(_read("brick_operator.hip"))
    assert "__global__" not in handle and "hipLaunchKernelGGL" not in handle  # no kernel, no launch
    uses = [ln.strip() for ln in handle.splitlines() if "->physics" in ln or "BOP_PHYSICS_" in ln]
    assert len(uses) >= 6
    for ln in uses:  # the ops table and the one-line create entry points
        assert ln.startswith(("static const BopOps ops[BOP_PHYSICS_ROWS + 1]", "/* BOP_PHYSICS_")) or ln == "return ops[op->physics];" or re.fullmatch(r"return bop_create\(ctx, m, BOP_PHYSICS_\w+, p, out\);", ln), ln
    assert "physics ==" not in handle and "physics !=" not in handle
    mg = _code(_read("brick_multigrid.hip"))
    for ln in mg.splitlines():
        if "BOP_PHYSICS_" in ln:  # the create entry points' tables: the message table's size and the physics each entry point builds hierarchies for
            assert "BOP_PHYSICS_ROWS" in ln or re.search(r'\{"mfem_brick_multigrid_create\w*", BOP_PHYSICS_\w+\}', ln), ln
        if "->physics" in ln:  # handed to a row lookup, the message table, the entry table's comparison or mg_refuse's name lookup: never compared with a tag
            assert re.search(r"(mg_wrong_physics|mg_refuse)\([^;]*->physics|->physics != E\.tag", ln), ln
    thermal = _read("brick_operator_thermal.hip")
    for kernel in ("k_brick_product_sweep", "k_brick_product_tiles", "k_brick_product_faces", "k_brick_diagonal"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", thermal), kernel
    for launcher in ("bop_thermal_launch", "bop_thermal_jacobi", "bop_thermal_signed_diagonal", "bop_view"):
        assert re.search(r"\bint " + launcher + r"\(", _read("brick_operator.h")), launcher

