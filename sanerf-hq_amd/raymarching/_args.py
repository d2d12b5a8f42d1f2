"""Tensor-argument helpers of the operator modules: what a binding does to a tensor before its pointer goes to the library."""
import torch

from .. import _lib


def _f32(t: torch.Tensor) -> torch.Tensor:
    """Detached, contiguous, float32 (the tensor itself where it already is)."""
    return t.detach().contiguous().float()


def _i64(t: torch.Tensor) -> torch.Tensor:
    """Detached, contiguous, int64 (labels, indices)."""
    return t.detach().contiguous().long()


def _flat3(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(-1, 3).contiguous().float()


def _row_view(t, name, rows=None, what="", channels=None, width=None, strided=True):
    """An [..., C] tensor as N rows of float32, read in place where its rows have unit stride and do not overlap (a column slice of a wider
    buffer), packed otherwise.  name: as the messages call it (None: no device check here, the caller's _lib.dev makes it behind its own
    shape checks); rows / what: the expected N and what it counts ("{N} rays"); channels: the allowed C; width: the leading columns the
    kernel reads (default all C; packing keeps only those); strided=False: for a kernel that takes no row stride, pack unless contiguous."""
    if name is not None and not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{name} must be a CUDA tensor")
    t = t.detach()
    if channels is not None and (t.dim() < 2 or t.shape[-1] not in channels):
        raise RuntimeError(f"{name} must be [N,{' or '.join(str(c) for c in channels)}], got {tuple(t.shape)}")
    if t.dim() != 2:
        t = t.reshape(-1, t.shape[-1])
    if rows is not None and t.shape[0] != rows:
        raise RuntimeError(f"{name}: {t.shape[0]} rows for {what}")
    w = t.shape[1] if width is None else width
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < w or t.shape[1] < w or not (strided or t.is_contiguous()):
        t = (t if width is None else t[:, :width]).float().contiguous()
    return t


def _image_rows(t, name, N):
    """An [N, >=3] float32 image whose rows are `stride` floats apart (the packed [N,5] render buffer's image columns are read in place)."""
    t = _row_view(t, name, N, f"{N} pixels", width=3)
    return t, t.data_ptr(), t.stride(0)


def _mask_rows(masks, labels):
    m = _row_view(masks, None, strided=False)
    lb = _i64(labels.reshape(-1))
    if lb.shape[0] != m.shape[0]:
        raise RuntimeError(f"{lb.shape[0]} labels for {m.shape[0]} mask rows")
    return m, lb


def _record_ptrs(record, workspace, record_bytes, workspace_bytes, kind):
    """The pointers of a meter's record and workspace, which must come from raymarching.{kind}_record() / {kind}_workspace()."""
    if record.dtype != torch.int64 or record.numel() * 8 < record_bytes:
        raise RuntimeError(f"record must come from raymarching.{kind}_record()")
    if workspace.dtype != torch.int64 or workspace.numel() * 8 < workspace_bytes:
        raise RuntimeError(f"workspace must come from raymarching.{kind}_workspace()")
    return _lib.dev(record, "record", torch.int64), _lib.dev(workspace, "workspace", torch.int64)


def _pixel_values(t, name, n):
    """n float32 values a constant number of floats apart, read in place: a contiguous tensor (1), or a column of the packed [N,5] render
    buffer such as buf[:, 3] or buf[:, 3].view(H, W) (5).  Anything else is packed first."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if t.numel() != n:
        raise RuntimeError(f"{name}: {t.numel()} values for {n} pixels")
    uniform = t.dim() >= 1 and t.stride(-1) >= 1 and all(t.stride(i) == t.stride(i + 1) * t.shape[i + 1] for i in range(t.dim() - 1))
    if not uniform:
        t = t.contiguous().reshape(-1)
    return t, t.data_ptr(), t.stride(-1)


def _i32(t, name, shape=None):
    """A contiguous int32 tensor on the device (labels, flags, coordinates; bool and int64 are converted by a device-side copy)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    t = t.detach()
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    t = t.contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _outputs(op, specs, want, out, dev):
    """The `out=` idiom of mask_output: name -> (shape, dtype); returns (dict of tensors, dict of pointers, None for an unwanted one)."""
    res, ptr = {} if out is None else out, {}
    for name, (shape, dtype) in specs.items():
        if name not in want:
            ptr[name] = None
            continue
        t = res.get(name)
        if t is None:
            t = res[name] = torch.empty(shape, device=dev, dtype=dtype)
        elif tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"{op}: out[{name!r}] must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}, "
                               f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        ptr[name] = _lib.dev(t, name, dtype)
    return res, ptr


def _f32_rows(t, name, cols=None):
    """A contiguous float32 [rows, cols] tensor on the device, read in place (nothing is copied: these are dataset or static tensors)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous float32 tensor, got {t.dtype}{'' if t.is_contiguous() else ' (not contiguous)'}")
    t = t.detach().reshape(-1, cols) if cols is not None else t.detach()
    return t


def _row_strided(t, name, rows, width, dtype):
    """(pointer, row stride in elements) of an output written in place: [rows] or [rows, >= width] with unit column stride -- a contiguous
    tensor or columns of a wider buffer (buf[:, 3:6], buf[:, 7])."""
    if not t.is_cuda:
        raise RuntimeError(f"out[{name!r}] must be a CUDA tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"out[{name!r}] must be a {dtype} tensor, got {t.dtype}")
    if t.dim() == 1 and width == 1:
        ok, stride = t.shape[0] == rows, t.stride(0)
    else:
        ok = t.dim() == 2 and t.shape[0] == rows and t.shape[1] == width and (t.stride(1) == 1 or width == 1)
        stride = t.stride(0) if t.dim() == 2 else 0
    if not ok or (rows > 1 and stride < width):
        raise RuntimeError(f"out[{name!r}] must be [{rows},{width}] with unit column stride and rows that do not overlap, got {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr(), max(int(stride), width)
