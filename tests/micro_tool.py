"""Where the GPU tests find tools/micro/bf16x6, the device check of the w16_* primitives (epnn_common.h): __graft_entry__.build()
compiles it with the library; a tree where it is missing gets it built here, by the same command."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bf16x6():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    if not os.path.exists(entry.MICRO):
        assert entry.build_micro(), "tools/micro/bf16x6 does not compile: the compiler's messages are on stderr"
    return entry.MICRO
