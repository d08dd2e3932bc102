"""The compiled submit/wait loops of libgck_driver.so (csrc/driver.cpp), driven without a GPU: the
library takes the engine's submit and wait entry points as pointers, so ctypes fakes stand in for
them, record every call and hand out the batch handles."""
import ctypes as C

import pytest

from gochugaru_amd import engine as E

_P = C.c_void_p
SUBMIT = C.CFUNCTYPE(C.c_int, _P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, C.c_int64, _P, _P, C.c_uint32, _P,
                     C.POINTER(_P))
SUBMIT_UNIFORM = C.CFUNCTYPE(C.c_int, _P, _P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, C.c_int64, _P, _P, C.c_size_t,
                             _P, C.POINTER(_P))
SUBMIT_SHAPED = C.CFUNCTYPE(C.c_int, _P, _P, _P, C.c_size_t, _P, _P, C.c_size_t, _P, _P, C.c_size_t, C.c_int64, _P, _P,
                            C.c_size_t, _P, C.POINTER(_P))
WAIT = C.CFUNCTYPE(C.c_int, _P, _P)

ENGINE, NOW, N, ERR_CAP = 0xE000, 1234567, 77, 5
KINDS = ("device", "host", "uniform", "shaped")


def _u64(xs):
    return (C.c_uint64 * max(1, len(xs)))(*xs)


class Loop:
    """One export of the driver over fake entry points. `events` holds ("s", k) per submit and
    ("w", k) per wait, `args` what submit k received after (engine, consistency); submit
    `fail_submit` / the wait of batch `fail_wait` return `code`."""

    def __init__(self, kind, n_batches, fail_submit=None, fail_wait=None, code=0):
        self.kind, self.k = kind, n_batches
        self.fail_submit, self.fail_wait, self.code = fail_submit, fail_wait, code
        self.events, self.args, self.live, self.max_live, self.waited = [], [], set(), 0, []
        # calls with a wrong engine, consistency or handle: an exception raised inside a ctypes
        # callback is only printed, so the callbacks record and run() asserts
        self.wrong = []
        self.cs = E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
        k = max(1, n_batches)
        col = lambda base: [base + 64 * i for i in range(k)]
        self.items, self.perm, self.err = col(0x100000), col(0x200000), col(0x300000)
        self.pairs, self.packed, self.errs = col(0x400000), col(0x500000), col(0x600000)
        self.shape_of, self.shapes = col(0x700000), col(0x800000)
        self.ns, self.n_shapes = [10 + i for i in range(k)], [1 + i % 64 for i in range(k)]
        self.streams = [0x900000 + 8 * i for i in range(8)]
        self.hdrs = (E.Uniform * k)()
        self.n_errs = (C.c_size_t * k)()
        self.wait_cb = WAIT(self._wait)
        proto = {"device": SUBMIT, "host": SUBMIT, "uniform": SUBMIT_UNIFORM, "shaped": SUBMIT_SHAPED}[kind]
        self.submit_cb = proto(self._submit)

    def _submit(self, e, cs, *rest):
        k = len(self.args)
        if (e, cs) != (ENGINE, C.addressof(self.cs)):
            self.wrong.append(("s", k, e, cs))
        self.events.append(("s", k))
        self.args.append(rest[:-1])
        if k == self.fail_submit:
            return self.code
        rest[-1][0] = 0xB000 + k  # the handle of batch k
        self.live.add(k)
        self.max_live = max(self.max_live, len(self.live))
        return 0

    def _wait(self, e, b):
        k = (b or 0) - 0xB000
        if e != ENGINE or k not in self.live:  # (a handle never given out, or waited for twice)
            self.wrong.append(("w", k, e, b))
        self.live.discard(k)
        self.waited.append(k)
        self.events.append(("w", k))
        return self.code if k == self.fail_wait else 0

    def run(self, depth, flags=0):
        drv = E._driver()
        secs = C.c_double(-1.0)
        head = (C.cast(self.submit_cb, _P), C.cast(self.wait_cb, _P), ENGINE, C.addressof(self.cs), self.k)
        if self.kind == "device":
            rc = drv.gckd_run(*head, _u64(self.items), _u64(self.perm), _u64(self.err), N, depth, _u64(self.streams),
                              flags, NOW, C.byref(secs))
        elif self.kind == "host":
            rc = drv.gckd_run_host(*head, _u64(self.items), _u64(self.perm), _u64(self.err), N, depth, NOW,
                                   C.byref(secs))
        elif self.kind == "uniform":
            rc = drv.gckd_run_uniform(*head, self.hdrs, _u64(self.pairs), _u64(self.ns), _u64(self.packed),
                                      _u64(self.errs), ERR_CAP, self.n_errs, depth, NOW, C.byref(secs))
        else:
            rc = drv.gckd_run_shaped(*head, _u64(self.shapes), _u64(self.n_shapes), _u64(self.shape_of),
                                     _u64(self.pairs), _u64(self.ns), _u64(self.packed), _u64(self.errs), ERR_CAP,
                                     self.n_errs, depth, NOW, C.byref(secs))
        self.seconds = secs.value
        assert not self.wrong, self.wrong
        return rc

    def order(self):
        return " ".join(f"{w}{k}" for w, k in self.events)


@pytest.mark.parametrize("kind", KINDS)
def test_depth_two_keeps_two_in_flight(kind):
    lp = Loop(kind, 5)
    assert lp.run(2) == E.GCK_OK
    assert lp.order() == "s0 s1 w0 s2 w1 s3 w2 s4 w3 w4"
    assert lp.max_live == 2 and not lp.live
    assert lp.seconds >= 0


@pytest.mark.parametrize("kind", KINDS)
def test_depth_zero_is_depth_one(kind):
    zero, one = Loop(kind, 4), Loop(kind, 4)
    assert zero.run(0) == E.GCK_OK and one.run(1) == E.GCK_OK
    assert zero.order() == one.order() == "s0 w0 s1 w1 s2 w2 s3 w3"
    assert zero.max_live == 1
    if kind == "device":  # streams[k % depth] with the depth the loop runs at
        assert [a[-1] for a in zero.args] == [zero.streams[0]] * 4


@pytest.mark.parametrize("kind", KINDS)
def test_depth_above_the_batches(kind):
    lp = Loop(kind, 3)
    assert lp.run(8) == E.GCK_OK
    assert lp.order() == "s0 s1 s2 w0 w1 w2"


@pytest.mark.parametrize("kind", KINDS)
def test_no_batches_no_calls(kind):
    lp = Loop(kind, 0)
    assert lp.run(2) == E.GCK_OK
    assert lp.events == [] and lp.seconds >= 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depth", (1, 2, 8))
def test_failed_submit_ends_the_loop(kind, depth):
    lp = Loop(kind, 6, fail_submit=3, code=3)
    assert lp.run(depth) == 3
    submits = [k for w, k in lp.events if w == "s"]
    assert submits == [0, 1, 2, 3]                  # none after the failed one
    assert sorted(lp.waited) == [0, 1, 2] and not lp.live  # every handle given out, exactly once


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depth", (1, 2, 8))
def test_failed_wait_ends_the_submits(kind, depth):
    lp = Loop(kind, 6, fail_wait=1, code=5)
    assert lp.run(depth) == 5
    submits = [k for w, k in lp.events if w == "s"]
    at = lp.events.index(("w", 1))
    assert all(w == "w" for w, _ in lp.events[at:])  # no submit follows the failed wait
    assert sorted(lp.waited) == submits and not lp.live  # the rest are waited for, exactly once


def test_device_loop_arguments():
    lp = Loop("device", 5)
    assert lp.run(2, flags=E.SUBMIT_ENGINE_STREAM) == E.GCK_OK
    for k, a in enumerate(lp.args):
        assert a == (lp.items[k], N, None, None, 0, NOW, lp.perm[k], lp.err[k],
                     E.SUBMIT_DEVICE | E.SUBMIT_ENGINE_STREAM, lp.streams[k % 2])
    lp = Loop("device", 2)
    assert lp.run(2) == E.GCK_OK
    assert [a[8] for a in lp.args] == [E.SUBMIT_DEVICE] * 2


def test_host_loop_arguments():
    lp = Loop("host", 5)
    assert lp.run(2) == E.GCK_OK
    for k, a in enumerate(lp.args):
        assert a == (lp.items[k], N, None, None, 0, NOW, lp.perm[k], lp.err[k], 0, None)


def test_uniform_loop_arguments():
    lp = Loop("uniform", 5)
    assert lp.run(2) == E.GCK_OK
    for k, a in enumerate(lp.args):
        assert a == (C.addressof(lp.hdrs) + k * C.sizeof(E.Uniform), lp.pairs[k], lp.ns[k], None, None, 0, NOW,
                     lp.packed[k], lp.errs[k], ERR_CAP, C.addressof(lp.n_errs) + k * C.sizeof(C.c_size_t))


def test_shaped_loop_arguments():
    lp = Loop("shaped", 5)
    assert lp.run(2) == E.GCK_OK
    for k, a in enumerate(lp.args):
        assert a == (lp.shapes[k], lp.n_shapes[k], lp.shape_of[k], lp.pairs[k], lp.ns[k], None, None, 0, NOW,
                     lp.packed[k], lp.errs[k], ERR_CAP, C.addressof(lp.n_errs) + k * C.sizeof(C.c_size_t))


@pytest.mark.parametrize("kind", KINDS)
def test_trace_stamps_of_a_successful_run(kind):
    n = 5
    stamps = (C.c_double * (2 * n))(*([-1.0] * (2 * n)))
    drv = E._driver()
    drv.gckd_set_trace(stamps, n)
    try:
        lp = Loop(kind, n)
        assert lp.run(2) == E.GCK_OK
    finally:
        drv.gckd_set_trace(None, 0)
    got = list(stamps)
    assert all(t >= 0 for t in got), got                        # every entry filled
    assert all(got[2 * k] <= got[2 * k + 1] for k in range(n)), got  # a batch's submit before its wait
    assert max(got) <= lp.seconds
