"""The place of the normal priority class kept for the process's null stream (include/epnn.h, "THE NULL STREAM'S PLACE"), and that
the library itself never uses that stream.  CPU only: the rule is a pure function, the sources are read as text."""
import ctypes as C
import glob
import os
import re

from conftest import ROOT


def _pick(live, limit, nclasses):
    from epnn_amd import _lib
    arr = (C.c_int * 3)(*live)
    return _lib.load().epnn_pick_stream_class(arr, limit, nclasses)


def _create(n, limit, nclasses, place):
    """The classes of n handles created in turn: what create_handle_stream passes to the rule (live[0] + place)."""
    tab, got = [0, 0, 0], []
    for _ in range(n):
        c = _pick([tab[0] + place, tab[1], tab[2]], limit, nclasses)
        assert 0 <= c < nclasses
        tab[c] += 1
        got.append(c)
    return got


# ------------------------------------------------------------------------------------------------ part 1: the placements
def test_no_place_five_eight_fourteen_handles():
    assert _create(5, 4, 3, 0) == [0, 0, 0, 0, 1]
    assert _create(8, 4, 3, 0) == [0, 0, 0, 0, 1, 1, 1, 1]
    # 4 + 4 + 4, then two that go to the emptiest class (the earlier one on a tie: normal, then high)
    assert _create(14, 4, 3, 0) == [0] * 4 + [1] * 4 + [2] * 4 + [0, 1]


def test_place_kept_five_eight_fourteen_handles():
    assert _create(5, 4, 3, 1) == [0, 0, 0, 1, 1]
    assert _create(8, 4, 3, 1) == [0, 0, 0, 1, 1, 1, 1, 2]
    # 3 + 4 + 4 and three that share (the null stream's place counts: every class holds four when the twelfth is asked for)
    assert _create(14, 4, 3, 1) == [0] * 3 + [1] * 4 + [2] * 4 + [0, 1, 2]


def test_sixteen_queues_keep_everything_normal_with_and_without_the_place():
    for place in (0, 1):
        for n in (5, 8, 14):
            assert _create(n, 16, 3, place) == [0] * n


def test_reserve_null_stream_checks_its_arguments():
    from epnn_amd import _lib
    lib = _lib.load()
    try:
        assert lib.epnn_reserve_null_stream(0, 1) == 0          # (no HIP call: works without a GPU)
        assert lib.epnn_reserve_null_stream(3, 0) == 0
        assert lib.epnn_reserve_null_stream(-1, 1) != 0
        assert b"device" in lib.epnn_last_error()
        assert lib.epnn_reserve_null_stream(0, 2) != 0
        assert b"0 or 1" in lib.epnn_last_error()
    finally:
        lib.epnn_reserve_null_stream(0, 0)                      # the default, for whatever this process creates later


# ------------------------------------------------------------------------------------------------ part 2: the sources
def _sources():
    out = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "epnn_amd", "csrc", "*"))):
        text = open(f).read()
        text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)      # comments out, lines kept
        text = re.sub(r"//[^\n]*", "", text)
        out[os.path.relpath(f, ROOT)] = text
    assert len(out) >= 20
    return out


def _calls(text, name_re):
    """(name, line number, [arguments]) of every call of a function whose name matches: arguments split at top-level commas."""
    for m in re.finditer(r"\b(" + name_re + r")\s*\(", text):
        depth, k, args, start = 1, m.end(), [], m.end()
        while depth and k < len(text):
            ch = text[k]
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
                if depth == 0:
                    args.append(text[start:k])
            elif ch == "," and depth == 1:
                args.append(text[start:k])
                start = k + 1
            k += 1
        assert depth == 0, (m.group(1), text.count("\n", 0, m.start()) + 1)
        yield m.group(1), text.count("\n", 0, m.start()) + 1, [" ".join(a.split()) for a in args]


_NULL = re.compile(r"^(\(\s*hipStream_t\s*\)\s*)?(0|nullptr|NULL|hipStreamLegacy|hipStream_t\s*\(\s*0?\s*\)|hipStream_t\s*\{\s*0?\s*\})$")


def test_no_synchronous_null_stream_call_in_the_sources():
    bad = []
    for f, text in _sources().items():
        for n, line in enumerate(text.splitlines(), 1):
            if re.search(r"\b(hipMemcpy|hipMemset|hipMemcpy2D|hipDeviceSynchronize)\s*\(", line):
                bad.append((f, n, line.strip()))
    assert not bad, bad


def test_no_async_call_or_launch_names_stream_zero():
    # where the stream is: index of the argument, and how many arguments the call has when it is given at all (HIP's C++ headers
    # default a missing stream to 0)
    where = {"hipMemcpyAsync": 4, "hipMemsetAsync": 3, "hipLaunchKernelGGL": 4, "hipEventRecord": 1, "hipGraphLaunch": 1,
             "hipStreamWaitEvent": 0, "hipStreamSynchronize": 0, "ncclAllReduce": 6, "ncclBroadcast": 6}
    bad, seen = [], 0
    for f, text in _sources().items():
        for name, line, args in _calls(text, r"hip\w*Async|hipLaunchKernelGGL|hipEventRecord|hipGraphLaunch|hipStreamWaitEvent|hipStreamSynchronize|ncclAllReduce|ncclBroadcast"):
            seen += 1
            if name not in where:
                bad.append((f, line, name, "an asynchronous call this test does not know: say where its stream is"))
            elif len(args) <= where[name]:
                bad.append((f, line, name, "no stream argument: it defaults to the null stream"))
            elif _NULL.match(args[where[name]]):
                bad.append((f, line, name, "stream " + args[where[name]]))
        if "<<<" in text:
            bad.append((f, 0, "<<<", "launches go through hipLaunchKernelGGL with a handle's stream"))
    assert seen > 300, seen                                       # (the scan sees the calls: ~200 launches, ~100 copies and fills)
    assert not bad, bad


def test_the_scan_catches_what_it_is_for():
    text = "void f() {\n  hipMemcpyAsync(a, b, n,\n      hipMemcpyHostToDevice);\n  hipMemsetAsync(p, 0, g(1, 2), 0);\n  hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, nullptr, x);\n  hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, h->stream, 0);\n}\n"
    got = list(_calls(text, r"hip\w*Async|hipLaunchKernelGGL"))
    assert [(n, l, len(a)) for n, l, a in got] == [("hipMemcpyAsync", 2, 4), ("hipMemsetAsync", 4, 4), ("hipLaunchKernelGGL", 5, 6), ("hipLaunchKernelGGL", 6, 6)]
    assert _NULL.match(got[1][2][3]) and _NULL.match(got[2][2][4]) and not _NULL.match(got[3][2][4])
    assert _NULL.match("(hipStream_t)0") and not _NULL.match("h->stream2") and not _NULL.match("st")
