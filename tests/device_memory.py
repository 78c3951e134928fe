"""Where the buffers of the shared kernel cases (sam_kernel_cases.py, fastq_cases.py) live: plain numpy arrays for the
CPU execution harness, CUDA tensors for the GPU.  Two objects with one interface, so that a case is written once and
runs on both.  TEST INFRASTRUCTURE ONLY.

    to_dev(array, shift=0)   the array's bytes in device memory, the first one `shift` bytes behind a 16-byte boundary,
                             with at least 16 readable bytes behind the last one (an empty array: one readable byte)
    zeros(n, dtype)          n zero entries, 16-byte aligned
    fill(buf, byte)          every byte of buf <- byte
    to_host(buf, dtype)      a numpy copy of the buffer's bytes, seen as dtype (default: bytes)
    sync()                   what the memory's own fills and copies need before the library may touch the buffers

The library works on a stream of its own that does not wait for torch's: GpuMemory.sync() is torch.cuda.synchronize(),
and every case calls sync() after its fills and before a library call (tests/test_gpu_approx.py device_tables records
the overwrite that a fill running late once caused)."""
import numpy as np


def _bytes_of(array):
    if isinstance(array, (bytes, bytearray)):
        return np.frombuffer(bytes(array), np.uint8)
    return np.ascontiguousarray(array).reshape(-1).view(np.uint8)


class HarnessMemory:
    """numpy arrays: the harness's kernels read and write host memory"""
    gpu = False

    def to_dev(self, array, shift=0):
        data = _bytes_of(array)
        raw = np.zeros(data.size + 64, np.uint8)
        at = (-raw.ctypes.data) % 16 + shift
        raw[at:at + data.size] = data
        return raw[at:at + max(data.size, 1)]

    def zeros(self, n, dtype=np.uint8):
        nbytes = int(n) * np.dtype(dtype).itemsize
        raw = np.zeros(nbytes + 32, np.uint8)
        at = (-raw.ctypes.data) % 16
        return raw[at:at + nbytes]

    def fill(self, buf, byte):
        buf[:] = byte

    def to_host(self, buf, dtype=np.uint8):
        return np.array(buf, copy=True).view(dtype)

    def sync(self):
        pass


class GpuMemory:
    """uint8 CUDA tensors (torch allocates, the library gets their addresses)"""
    gpu = True

    def __init__(self):
        import torch
        self.torch = torch

    def to_dev(self, array, shift=0):
        torch = self.torch
        data = _bytes_of(array)
        raw = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda")
        at = (-raw.data_ptr()) % 16 + shift
        if data.size:
            raw[at:at + data.size] = torch.from_numpy(data.copy()).cuda()
        return raw[at:at + max(data.size, 1)]

    def zeros(self, n, dtype=np.uint8):
        torch = self.torch
        nbytes = int(n) * np.dtype(dtype).itemsize
        raw = torch.zeros(nbytes + 32, dtype=torch.uint8, device="cuda")
        at = (-raw.data_ptr()) % 16
        return raw[at:at + nbytes]

    def fill(self, buf, byte):
        buf.fill_(byte)

    def to_host(self, buf, dtype=np.uint8):
        return buf.cpu().numpy().copy().view(dtype)

    def sync(self):
        self.torch.cuda.synchronize()
