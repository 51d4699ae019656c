"""(no GPU) The device check of the bf16 split arithmetic, tools/micro/bf16x6, runs the shipped primitives and not copies of them: a
layout test on source text and on the build command.  The matrix-pipe builtins and the v_perm_b32 selector of the w16_* primitives
occur in one file of the library, epnn_common.h; the tool includes that file and has none of them itself; it is compiled with every
flag of the library; and a tool that does not compile is reported, not raised."""
import os
import re

import __graft_entry__ as entry
from conftest import ROOT

SHIPPED = ("mfma_f32_16x16x32_bf16", "mfma_f32_4x4x4", "0x07060302")
TOOL = os.path.join(ROOT, "tools", "micro", "bf16x6.hip")


def _text(path):
    with open(path) as f:
        return f.read()


def test_the_tool_includes_the_primitives_and_copies_none():
    src = _text(TOOL)
    assert re.search(r'^#include "epnn_common\.h"$', src, re.M)
    for s in SHIPPED:
        assert s not in src, s
    # (none of its earlier copies is defined again; the comparison arms it keeps have other names)
    for name in ("pack_hi", "pack_hi2", "ident4", "mm4", "mm", "split3", "split3q", "split3k16_valu"):
        assert not re.search(r"\b%s\(" % name, src), name
    for t in ("f32x4", "f32x2", "u32x4"):
        assert not re.search(r"typedef[^;\n]*\b%s\b" % t, src), t


def test_the_shipped_builtins_are_in_one_file():
    # as builtins or as the selector: comments name the instructions (v_mfma_f32_...) in every file
    shipped = ["__builtin_amdgcn_" + s for s in SHIPPED[:2] + ("perm(", "permlane16_swap", "permlane32_swap")] + [SHIPPED[2]]
    texts = {f: _text(os.path.join(entry.CSRC, f)) for f in sorted(os.listdir(entry.CSRC))}
    for s in shipped:
        assert [f for f, src in texts.items() if s in src] == ["epnn_common.h"], s


def test_the_tool_is_compiled_with_the_library_s_flags():
    cmd = entry.micro_command()
    assert cmd[0] == entry.HIPCC
    for flag in entry.BUILD_FLAGS:
        assert flag in cmd, flag
    assert cmd[cmd.index("-I") + 1] == entry.CSRC
    assert cmd[cmd.index("-o") + 1] == os.path.join(ROOT, "tools", "micro", "bf16x6") and cmd[-1] == TOOL


def test_a_tool_that_does_not_compile_is_not_fatal(capfd):
    hipcc = entry.HIPCC
    entry.HIPCC = "/bin/false"
    try:
        assert entry.build_micro(force=True) is False
    finally:
        entry.HIPCC = hipcc
    assert "bf16x6 was not built" in capfd.readouterr().err
