"""querytext.model_query_vectors, the plain statement of rr_query_vectors_dev, against the expression QueryEncoder.encode_ids
normalises with, as uint32 bit patterns.  This is the proof that the stated order of the additions is numpy's at every
width class of its pairwise split (below 8, the eight-accumulator block with and without a tail, one split, two, six) and
that the maximum, the square root and the quotients round as numpy's do at the edges of the float32 range."""
import numpy as np
import pytest

from query_vector_cases import WIDTHS, assert_bitwise, numpy_vectors, rows_of

from review_recommender_amd.querytext import PAIRWISE_BLOCK, model_pairwise_leaves, model_query_vectors


@pytest.mark.parametrize("dim", WIDTHS)
def test_model_equals_numpy_bitwise(dim):
    e = rows_of(dim)
    assert_bitwise(model_query_vectors(e), numpy_vectors(e))


def test_rows_cover_the_edges_they_are_named_for():
    e = rows_of(384)
    want = numpy_vectors(e)
    with np.errstate(all="ignore"):
        norm = np.linalg.norm(e, axis=1)
        sq = e * e
    names = {"zero": 3, "tiny": 4, "huge": 5, "nan": 6, "inf": 7, "signs": 8}
    assert not e[names["zero"]].any() and not want[names["zero"]].any()
    assert norm[names["tiny"]] < np.float32(1e-12) and e[names["tiny"]].any()
    assert (sq[names["tiny"]] < np.finfo(np.float32).tiny).all()                  # denormal or zero squares
    assert np.isinf(norm[names["huge"]]) and np.isfinite(e[names["huge"]]).all() and not want[names["huge"]].any()
    assert np.isnan(want[names["nan"]]).all()                                     # numpy's maximum keeps the NaN norm
    assert np.isnan(want[names["inf"]]).sum() == 1 and (want[names["inf"]][np.isfinite(e[names["inf"]])] == 0).all()
    assert (np.sign(e[names["signs"]][:-1]) == -np.sign(e[names["signs"]][1:])).all()


def test_leaves_are_the_split_the_kernel_walks():
    """The limits csrc/rr_query.hip sizes its tables by: at most 128 pieces and seven splits deep up to dim 8192, every piece
    of 64 .. 128 terms once there is a split, and for dim 384 four pieces of 96."""
    assert model_pairwise_leaves(384) == [(0, 96, 2), (96, 96, 2), (192, 96, 2), (288, 96, 2)]
    assert model_pairwise_leaves(7) == [(0, 7, 0)] and model_pairwise_leaves(128) == [(0, 128, 0)]
    assert model_pairwise_leaves(129) == [(0, 64, 1), (64, 65, 1)]
    most = deepest = 0
    for n in range(1, 8193):
        leaves = model_pairwise_leaves(n)
        assert sum(m for _, m, _ in leaves) == n and [f for f, _, _ in leaves] == list(np.cumsum([0] + [m for _, m, _ in leaves[:-1]]))
        if n > PAIRWISE_BLOCK:
            assert all(64 <= m <= PAIRWISE_BLOCK for _, m, _ in leaves)
        most, deepest = max(most, len(leaves)), max(deepest, max(d for _, _, d in leaves))
    assert len(model_pairwise_leaves(8192)) == 64 and most <= 128 and deepest <= 7
