"""The rule that places a handle's stream in a priority class (include/epnn.h at epnn_create; epnn_host.h pick_stream_class),
called through the C ABI.  CPU only: the function makes no HIP call."""
import ctypes as C


def _pick(live, limit, nclasses):
    from epnn_amd import _lib
    arr = (C.c_int * 3)(*live)
    return _lib.load().epnn_pick_stream_class(arr, limit, nclasses)


def _fill(n, limit, nclasses):
    live, got = [0, 0, 0], []
    for _ in range(n):
        c = _pick(live, limit, nclasses)
        assert 0 <= c < nclasses
        live[c] += 1
        got.append(c)
    return got, live


def test_four_queues_three_classes_fill_in_order_then_share_evenly():
    got, live = _fill(18, 4, 3)
    assert got == [0] * 4 + [1] * 4 + [2] * 4 + [0, 1, 2, 0, 1, 2]
    assert live == [6, 6, 6]


def test_eight_lanes_are_four_normal_four_high():
    assert _fill(8, 4, 3)[0] == [0, 0, 0, 0, 1, 1, 1, 1]


def test_one_class_is_always_normal():
    assert _fill(11, 4, 1)[0] == [0] * 11


def test_two_classes_never_give_the_third():
    assert _fill(11, 4, 2)[0] == [0] * 4 + [1] * 4 + [0, 1, 0]


def test_plentiful_queues_change_nothing():
    assert _fill(14, 16, 3)[0] == [0] * 14


def test_limit_of_one():
    assert _fill(7, 1, 3)[0] == [0, 1, 2, 0, 1, 2, 0]
    assert _fill(3, 1, 1)[0] == [0, 0, 0]
    assert _pick([0, 0, 0], 0, 3) == 0 and _pick([1, 0, 0], 0, 3) == 1       # a limit below 1 counts as 1


def test_a_place_given_back_is_the_next_taken():
    assert _pick([3, 4, 0], 4, 3) == 0
    assert _pick([4, 3, 0], 4, 3) == 1
    assert _pick([4, 4, 3], 4, 3) == 2
    assert _pick([5, 4, 4], 4, 3) == 1                                       # all full: the fewest, the earlier class on a tie
    assert _pick([4, 4, 4], 4, 3) == 0
