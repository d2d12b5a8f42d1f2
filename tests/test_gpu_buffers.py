"""sanerf_hq_amd._buffers on the device: the library's zero fill and the two workspace caches that ops.py and raymarching/ share."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [0, 3, 4, 1024])          # 3 floats = 12 bytes: no multiple of 16, torch's fill; the others: sn_zero (0: nothing)
def test_zero_fill(gpu, n):
    from sanerf_hq_amd import _buffers
    torch.empty(n, device=gpu).fill_(7.0)                 # (what the allocator hands out next is not zero by luck)
    t = _buffers.zeros_f32((n,), gpu)
    assert t.shape == (n,) and t.dtype == torch.float32 and t.device == gpu
    assert int((t != 0).sum()) == 0


def test_zero_fill_unaligned_pointer(gpu):
    """zeros_f32 allocates its own tensor, so only the allocator can hand it a pointer that is not 16-byte aligned."""
    from sanerf_hq_amd import _buffers
    odd = [torch.empty(k, device=gpu, dtype=torch.uint8) for k in (1, 3, 5, 7)]     # odd-sized neighbours: the only lever there is
    ts = [_buffers.zeros_f32((4 * k,), gpu) for k in (1, 2, 3)]
    unaligned = [t for t in ts if t.data_ptr() % 16]
    del odd
    if not unaligned:
        pytest.skip("torch's caching allocator rounds every block to 512 bytes: it cannot be made to yield a pointer that is not 16-byte aligned")
    assert all(int((t != 0).sum()) == 0 for t in unaligned)


def test_scratch(gpu):
    from sanerf_hq_amd import _buffers
    a = _buffers.scratch("test_a", gpu, 1000)
    assert a.dtype == torch.uint8 and a.device == gpu and a.numel() >= 1000
    assert _buffers.scratch("test_a", gpu, 1000).data_ptr() == a.data_ptr()
    assert _buffers.scratch("test_a", gpu, 10).data_ptr() == a.data_ptr()           # large enough: kept
    b = _buffers.scratch("test_b", gpu, 1000)
    assert b.data_ptr() != a.data_ptr()                                              # another tag: another buffer
    grown = _buffers.scratch("test_a", gpu, 5000)
    assert grown.numel() >= 5000 and _buffers.scratch("test_a", gpu, 5000) is grown
    assert _buffers.scratch("test_b", gpu, 1000) is b
    floored = _buffers.scratch("test_floor", gpu, 100, floor=1 << 12)
    assert floored.numel() == 1 << 12
    assert _buffers.scratch("test_floor", gpu, 1 << 12, floor=1 << 12) is floored    # the floor saved this reallocation
    assert _buffers.scratch("test_floor", gpu, 1 << 13, floor=1 << 12).numel() == 1 << 13


def test_zeroed(gpu):
    from sanerf_hq_amd import _buffers
    main = torch.cuda.current_stream(gpu).cuda_stream
    side = torch.cuda.Stream(gpu)
    a = _buffers.zeroed("test_z", gpu, main, 256)
    assert a.dtype == torch.int64 and a.numel() * 8 >= 256 and int((a != 0).sum()) == 0
    assert _buffers.zeroed("test_z", gpu, main, 256) is a and _buffers.zeroed("test_z", gpu, main, 8) is a
    b = _buffers.zeroed("test_z", gpu, side.cuda_stream, 256)
    assert b is not a and b.data_ptr() != a.data_ptr()                               # one per stream
    assert _buffers.zeroed("test_other", gpu, main, 256) is not a                    # and per tag
    a.fill_(-1)                                                                      # (a kernel that broke zero-at-rest)
    grown = _buffers.zeroed("test_z", gpu, main, 4096)
    assert grown is not a and grown.numel() * 8 >= 4096 and int((grown != 0).sum()) == 0
    assert _buffers.zeroed("test_z", gpu, side.cuda_stream, 256) is b
