"""flooder_selftest writes the 128 floats its header promises and nothing behind them (it used to write 64 more, into
whatever tensor the allocator had placed next).  Runs on a real MI355X only (-m gpu)."""
import pytest
import torch

from flooder_amd import _native

pytestmark = pytest.mark.gpu


def test_selftest_stays_inside_its_output_buffer():
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    lib = _native.load()
    dev = torch.device("cuda:0")
    x = torch.rand(64, generator=torch.Generator().manual_seed(3))
    buf = torch.full((512,), -7.0, device=dev)
    out = buf[128:256]                                   # guard words on both sides
    assert lib.flooder_selftest(_native.ptr(x.to(dev)), out.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got[128:192], torch.full((64,), float(x.min())))
    assert torch.equal(got[192:256], torch.full((64,), float(x.max())))
    assert torch.equal(got[:128], torch.full((128,), -7.0)) and torch.equal(got[256:], torch.full((256,), -7.0))
