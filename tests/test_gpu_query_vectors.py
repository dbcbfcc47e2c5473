"""rr_query_vectors_dev (csrc/rr_query.hip) against the expression QueryEncoder.encode_ids normalises with, as uint32 bit
patterns: every width class of numpy's pairwise split, batches around a wave's 64 lanes and beyond one pass of eight pieces,
rows at the edges of the float32 range; in place, with flagged rows, empty and refused calls."""
import ctypes as C

import numpy as np
import pytest

from query_vector_cases import WIDTHS, assert_bitwise, batch_of, numpy_vectors

pytestmark = pytest.mark.gpu

EPS = 1e-12
SENTINEL = 7.0


def vectors(hip, e, needs=None, in_place=False):
    """The kernel over ``e`` (n, dim): the output on the host; without ``in_place`` into a buffer filled with SENTINEL."""
    import torch
    n, dim = e.shape
    d = torch.from_numpy(np.ascontiguousarray(e, dtype=np.float32)).cuda()
    out = d if in_place else torch.full((n, dim), SENTINEL, dtype=torch.float32, device="cuda")
    flags = torch.from_numpy(np.ascontiguousarray(needs, dtype=np.int32)).cuda() if needs is not None else None
    rc = hip.rr_query_vectors_dev(C.c_void_p(d.data_ptr()), n, dim, EPS, C.c_void_p(flags.data_ptr()) if needs is not None else None,
                                  C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip.rr_last_error()
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(d.view(torch.int32).cpu(), torch.from_numpy(np.ascontiguousarray(e)).view(torch.int32))   # input untouched
    return out.cpu().numpy()


@pytest.mark.parametrize("dim", WIDTHS)
def test_kernel_equals_numpy_bitwise(hip, dim):
    for n in (1, 2, 63, 64, 65, 257):
        e = batch_of(dim, n)
        assert_bitwise(vectors(hip, e), numpy_vectors(e))


@pytest.mark.parametrize("dim", [7, 129, 384, 1000])
def test_in_place(hip, dim):
    e = batch_of(dim, 65)
    assert_bitwise(vectors(hip, e, in_place=True), numpy_vectors(e))


@pytest.mark.parametrize("dim", [9, 384, 1024])
def test_flagged_rows_are_zeros_and_the_others_untouched_arithmetic(hip, dim):
    n = 65
    e = batch_of(dim, n)
    e[[0, 31, n - 1]] = batch_of(dim, 12)[[9, 10, 11]]                   # finite rows where the flags go
    needs = np.zeros(n, dtype=np.int32)
    needs[0], needs[31], needs[n - 1] = 1, 32, 5
    want = numpy_vectors(e)
    assert (want[[0, 31, n - 1]] != 0).any(axis=1).all()
    want[[0, 31, n - 1]] = 0
    for in_place in (False, True):
        got = vectors(hip, e, needs, in_place)
        assert_bitwise(got, want)
        assert not got[[0, 31, n - 1]].view(np.uint32).any()             # +0.0, every bit


def test_no_queries_and_refused_calls(hip):
    import torch
    d = torch.full((4, 384), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full((4, 384), SENTINEL, dtype=torch.float32, device="cuda")
    p, o, st = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip.rr_query_vectors_dev(p, 0, 384, EPS, None, o, st) == 0
    for args in ((p, -1, 384, EPS, None, o, st), (p, 65536, 384, EPS, None, o, st), (p, 4, 0, EPS, None, o, st),
                 (p, 4, 8193, EPS, None, o, st), (None, 4, 384, EPS, None, o, st), (p, 4, 384, EPS, None, None, st),
                 (p, 4, 384, float("nan"), None, o, st), (None, 0, 384, EPS, None, None, st)):
        assert hip.rr_query_vectors_dev(*args) == -1, args
        assert b"rr_query_vectors_dev" in hip.rr_last_error()
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    f = C.c_void_p(flags.data_ptr())
    for args in ((None, 4, 32, f, st), (f, 4, 32, None, st), (f, -1, 32, f, st), (f, 4, 0, f, st), (f, 4, 48, f, st)):
        assert hip.rr_query_flag_dev(*args) == -1, args
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((d == SENTINEL).all())     # nothing was launched


def test_flag_call_sets_one_bit(hip):
    import torch
    src = torch.tensor([0, 1, 0, 7, -1] * 30, dtype=torch.int32, device="cuda")     # 150 queries: three workgroups
    flags = torch.tensor([0, 0, 5, 5, 32] * 30, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip.rr_query_flag_dev(C.c_void_p(src.data_ptr()), 150, 32, C.c_void_p(flags.data_ptr()), st) == 0
    assert hip.rr_query_flag_dev(C.c_void_p(src.data_ptr()), 0, 32, C.c_void_p(flags.data_ptr()), st) == 0
    assert flags.cpu().tolist() == [0, 32, 5, 37, 32] * 30
