"""Named, zeroed arrays where the library's kernels of one context can reach them."""
import numpy as np


class DeviceBuffers:
    """f64 / i64: {name: shape} of float64 / int64 arrays.  On the GPU build they are torch-ROCm tensors on the context's
    device (the library works on their pointers; one synchronise after allocation), under the emulation build of the
    tests, whose "device" is host memory, numpy arrays."""

    def __init__(self, ctx, f64=None, i64=None):
        self._dev = None
        if ctx.on_gpu:
            import torch
            self._torch, self._dev = torch, torch.device("cuda", ctx.device)
            new = lambda s, t: torch.zeros(s, dtype=getattr(torch, t), device=self._dev)  # noqa: E731
        else:
            new = lambda s, t: np.zeros(s, dtype=t)  # noqa: E731
        self._buf = {k: new(s, "float64") for k, s in (f64 or {}).items()}
        self._buf.update({k: new(s, "int64") for k, s in (i64 or {}).items()})
        self.sync()

    def __contains__(self, name):
        return name in self._buf

    def ptr(self, name):
        """The array's device address; None for a name that is not held (an optional output the library may skip)."""
        a = self._buf.get(name)
        if a is None:
            return None
        return a.ctypes.data if self._dev is None else a.data_ptr()

    def array(self, name):
        """The tensor or ndarray itself (device-side slicing and column copies)."""
        return self._buf[name]

    def host(self, name):
        """A host copy as a numpy array."""
        a = self._buf[name]
        return a.copy() if self._dev is None else a.cpu().numpy()

    def sync(self):
        """Wait for the torch stream's work on the buffers (the library works on a stream of its own)."""
        if self._dev is not None:
            self._torch.cuda.synchronize(self._dev)
