"""The document-bound helpers on the device give what they give on the host (they are plain torch: cummax, cummin,
searchsorted and gather on HIP tensors), on the layouts a document-masked attention would be tested with."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _random_lengths(S, seed):
    g = torch.Generator().manual_seed(seed)
    out, left = [], S
    while left > 0:
        n = min(left, int(torch.randint(1, 200, (1,), generator=g)))
        out.append(n)
        left -= n
    return out


LAYOUTS = {
    "s320": [[1, 63, 64, 65, 127]],                    # a one-token document, boundaries on and off 64 and 128
    "s512": [[300, 212]],
    "s1000": [_random_lengths(1000, 11)],              # ragged
    "b2": [[384], [5, 59, 1, 127, 64, 100, 28]],       # row 0 one document, row 1 many
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_device_equals_host(name):
    from picotron_amd import ops
    lengths = LAYOUTS[name]
    S = sum(lengths[0])
    host = ops.doc_starts_from_lengths(lengths, S, check=True)
    dev = ops.doc_starts_from_lengths(lengths, S, check=True, device=DEV)
    assert dev.is_cuda and dev.dtype == torch.int32
    assert torch.equal(dev.cpu(), host)
    assert torch.equal(ops.doc_bounds(dev).cpu(), ops.doc_bounds(host))
    # the same rows written as tokens: an EOS closes every document
    ids = torch.full((len(lengths), S), 7, dtype=torch.int64)
    for b, row in enumerate(lengths):
        end = 0
        for n in row:
            end += n
            ids[b, end - 1] = 2
    assert torch.equal(ops.doc_starts_from_eos(ids.to(DEV), 2).cpu(), host)
    assert ops.check_doc_start(dev)
