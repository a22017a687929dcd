"""The argument checks and result exits the wrappers share: one definition, and one copy of the message, of each."""
import ctypes as C

import numpy as np

from ._abi import _ptr


def region(origin, dims):
    """origin and dims of a region (cells at max_depth, x y z) -> (origin, dims) as lists of int, and as the int32[3] the calls take"""
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    return o, n, (C.c_int32 * 3)(*o), (C.c_int32 * 3)(*n)


def region_shape(n):
    """[nz, ny, nx] of a region of dims n; an extent below 0 is none"""
    return [max(v, 0) for v in reversed(n)]


def region_cells(n):
    nz, ny, nx = region_shape(n)
    return nz * ny * nx


def device_i32(a, what, width=None):
    """an array, or an int32 cuda tensor (`what` names it in the refusal of any other tensor) -> a contiguous int32 cuda tensor:
    rows of `width` ([n, 3] cells, [n, 6] segments), or with width None as it is shaped"""
    import torch
    if isinstance(a, torch.Tensor):
        if not a.is_cuda or a.dtype != torch.int32:
            raise ValueError("a %s tensor is int32 on the device" % what)
        return (a if width is None else a.reshape(-1, width)).contiguous()
    a = np.asarray(a, np.int32)
    return torch.from_numpy(np.ascontiguousarray(a if width is None else a.reshape(-1, width))).cuda()


def device_rows(a, torch_dtype, np_dtype, width, what):
    """a cuda tensor of that type as it is, anything else uploaded: -> a contiguous [rows, width] cuda tensor"""
    import torch
    if isinstance(a, torch.Tensor):
        if not a.is_cuda or a.dtype != torch_dtype:
            raise ValueError("a %s tensor is %s on the device" % (what, str(torch_dtype).replace("torch.", "")))
        return a.reshape(-1, width).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np_dtype).reshape(-1, width))).cuda()


def field_i32(field, n):
    """a field over dims n, an array or an int32 cuda tensor -> a contiguous int32 cuda tensor"""
    t_field = device_i32(field, "field")
    if t_field.numel() != region_cells(n):
        raise ValueError("the field holds dims[0] * dims[1] * dims[2] values")
    return t_field


def ptr_or_null(t):
    """the tensor's device pointer; NULL for None and for a tensor without elements"""
    return _ptr(t) if t is not None and t.numel() else None


def stats_dict(st):
    """a stats struct -> {field: int}, by the struct's own _fields_"""
    return {name: int(getattr(st, name)) for name, _ in st._fields_}


def result(out, as_tensor=False):
    """the exit of a wrapper: cuda tensors as they are with as_tensor, else numpy arrays; a tuple or a dict entry by entry, None
    stays None"""
    if as_tensor or out is None:
        return out
    if isinstance(out, tuple):
        return tuple(result(v) for v in out)
    if isinstance(out, dict):
        return {name: result(v) for name, v in out.items()}
    return out.cpu().numpy()


class Outputs:
    """The named outputs of one call.  `fields`: {name: (torch dtype, numpy dtype of the result)} of every output the call has, in
    the order of its arguments; `want`: the names to compute -- the others are passed as NULL."""

    def __init__(self, fields, want):
        self.fields, self.names, self.bufs = fields, tuple(want), {}
        for name in self.names:
            if name not in fields:
                raise KeyError("no output %r (have: %s)" % (name, ", ".join(fields)))

    def alloc(self, shape, **shapes):
        """a device buffer of `shape` for every wanted name; `shapes`: the names that have a shape of their own"""
        import torch
        for name in self.names:
            self.bufs[name] = torch.empty(shapes.get(name, shape), dtype=self.fields[name][0], device="cuda")

    def ptrs(self):
        """one pointer per field, in field order"""
        return [_ptr(self.bufs.get(name)) for name in self.fields]

    def result(self, as_tensor=False):
        """the wanted outputs: the cuda tensors, or numpy arrays viewed as the field's numpy dtype (torch has no uint32 / uint64)"""
        if as_tensor:
            return {name: self.bufs[name] for name in self.names}
        return {name: self.bufs[name].cpu().numpy().view(self.fields[name][1]) for name in self.names}
