"""Document bounds of packed rows (ops.doc_starts_from_eos / doc_starts_from_lengths / doc_bounds), no GPU: against a
Python loop, and the mask they describe read from the query and from the key side."""
import pytest
import torch

EOS = 2


def _loop_starts(row, eos):
    """a token that follows an EOS opens a new document, and token 0 always does"""
    out, cur = [], 0
    for i in range(len(row)):
        if i == 0 or row[i - 1] == eos:
            cur = i
        out.append(cur)
    return out


def _loop_ends(starts):
    """one past the last token of the document that holds token i"""
    S = len(starts)
    out = []
    for i in range(S):
        j = i + 1
        while j < S and starts[j] == starts[i]:
            j += 1
        out.append(j)
    return out


ROWS = {
    "eos_at_0": [EOS, 5, 6, 7, EOS, 8, 9, 3],
    "eos_at_last": [4, 5, 6, EOS, 7, 8, 9, EOS],
    "consecutive_eos": [4, EOS, EOS, EOS, 5, 6, EOS, 7],
    "no_eos": [4, 5, 6, 7, 8, 9, 3, 1],
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_doc_starts_and_bounds_match_a_python_loop(name):
    from picotron_amd import ops
    row = ROWS[name]
    # two rows per batch: the case, and the case reversed (another layout in the same call)
    ids = torch.tensor([row, row[::-1]], dtype=torch.int64)
    start = ops.doc_starts_from_eos(ids, EOS)
    assert start.dtype == torch.int32 and tuple(start.shape) == (2, len(row))
    want = [_loop_starts(r, EOS) for r in (row, row[::-1])]
    assert start.tolist() == want
    assert ops.check_doc_start(start)
    bounds = ops.doc_bounds(start)
    assert bounds.dtype == torch.int32 and tuple(bounds.shape) == (2, 2, len(row)) and bounds.is_contiguous()
    assert bounds[0].tolist() == want
    assert bounds[1].tolist() == [_loop_ends(w) for w in want]
    # the mask read from both sides is one mask: doc_start[i] <= j <= i  <=>  j <= i < doc_end[j]; every row sees
    # at least itself
    for b in range(2):
        s, e = bounds[0, b].tolist(), bounds[1, b].tolist()
        for i in range(len(row)):
            assert s[i] <= i < e[i]
            for j in range(len(row)):
                assert (s[i] <= j <= i) == (j <= i < e[j])


def test_doc_bounds_accepts_int64_and_refuses_other_input():
    from picotron_amd import ops
    start = torch.tensor([[0, 0, 2, 2, 4]], dtype=torch.int64)
    bounds = ops.doc_bounds(start)
    assert bounds.dtype == torch.int32 and bounds.tolist() == [[[0, 0, 2, 2, 4]], [[2, 2, 4, 4, 5]]]
    assert ops.doc_bounds(torch.zeros(1, 1, dtype=torch.int32)).tolist() == [[[0]], [[1]]]
    with pytest.raises(ValueError):
        ops.doc_bounds(start.float())
    with pytest.raises(ValueError):
        ops.doc_bounds(start[0])
    with pytest.raises(ValueError):
        ops.doc_starts_from_eos(torch.tensor([1, 2, 3]), EOS)


def test_doc_starts_from_lengths():
    from picotron_amd import ops
    start = ops.doc_starts_from_lengths([[1, 3, 4], [8]], 8)
    assert start.dtype == torch.int32
    assert start.tolist() == [[0, 1, 1, 1, 4, 4, 4, 4], [0] * 8]
    assert ops.doc_starts_from_lengths([2, 0, 3], 5, check=True).tolist() == [[0, 0, 2, 2, 2]]
    lengths = torch.tensor([[1, 63, 64, 65, 127]])
    got = ops.doc_starts_from_lengths(lengths, 320, check=True)[0].tolist()
    want = []
    for n in lengths[0].tolist():
        want += [len(want)] * n
    assert got == want
    with pytest.raises(ValueError):
        ops.doc_starts_from_lengths([[3, 4]], 8, check=True)
    assert ops.check_doc_start(start)
    assert not ops.check_doc_start(torch.tensor([[0, 2, 1, 1]], dtype=torch.int32))  # 2 > its index
    assert not ops.check_doc_start(torch.tensor([[0, 1, 0, 3]], dtype=torch.int32))  # decreasing
    assert not ops.check_doc_start(torch.tensor([[1, 1, 1, 1]], dtype=torch.int32))  # token 0 opens no document


def test_eos_and_lengths_agree():
    from picotron_amd import ops
    lengths = [[3, 1, 4], [8]]
    ids = torch.full((2, 8), 7, dtype=torch.int64)
    ids[0, 2] = ids[0, 3] = ids[0, 7] = EOS  # the last token of each document of row 0
    ids[1, 7] = EOS
    assert torch.equal(ops.doc_starts_from_eos(ids, EOS), ops.doc_starts_from_lengths(lengths, 8))
