"""GPU: ``_native.launch`` on a real entry point -- the kernel runs on the current stream of the device it is given, the current device stays what
it was, the call is counted once, and a refusal of the entry point's own argument check is raised under its name and still counted."""
import pytest
import torch

from pytorch_toolbelt_amd import _native as N

pytestmark = pytest.mark.gpu


def test_launch_runs_ptb_merge_div_on_the_current_stream():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    image = torch.arange(-8, 8, dtype=torch.float32, device=dev) * 0.37
    norm = torch.tensor([1.0, 2.0, 4.0, 8.0] * 4, device=dev)             # (powers of two: the quotient is exact whatever the divide rounds like)
    out = torch.full((16,), -1.0, device=dev)
    want = image / norm
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    current = torch.cuda.current_device()
    with torch.cuda.stream(side):
        before = N.calls
        assert N.launch("ptb_merge_div", dev, image.data_ptr(), norm.data_ptr(), out.data_ptr(), 1, 16) is None
        assert N.calls == before + 1
        assert torch.cuda.current_device() == current
        with pytest.raises(RuntimeError, match="ptb_merge_div: invalid argument"):       # C = 0: refused before anything is launched
            N.launch("ptb_merge_div", dev, image.data_ptr(), norm.data_ptr(), out.data_ptr(), 0, 16)
        assert N.calls == before + 2
        assert torch.cuda.current_device() == current
    side.synchronize()
    assert torch.equal(out, want)
