"""ImagingIO — modules/imaging_IO.py of the reference with the record's smoothing and scaling on the device.

  get_file_list / get_time_from_file_path   :8-20   (host)
  ImagingIO.__getitem__                     :37-48  _read_das_npz (host: file reading, channel and taper cut), then
                                                    savgol_filter(data, 21, 15) and ``data /= scale`` in one pass of
                                                    dvh_savgol_rows (preprocess.savgol_smooth); with smoothing=False
                                                    the division alone (dvh_divide_rows)

``data`` comes back as a device tensor in the record's dtype (float32 and float64 are kept, anything else is converted
to float64 on the host, as savgol_filter does); the axes are the file's NumPy arrays, cut.  Constructing the object,
listing the files and get_time_interval do not touch the device.  Two keywords beyond the reference's: ``device``
(None: the current device at the first read) and ``prefetch``: iterating with prefetch=1 reads and uploads record
k + 1 on a background thread, through a pinned buffer and a side stream, while record k is in use; prefetch=0 reads
in line.  Both give the tensors ``io[k]`` gives, bit for bit.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
from datetime import datetime

import numpy as np
import torch

from .utils import _read_das_npz

SCALE_AFTER_DATE = "20230219"  # date folders after this one are divided by SCALE (:41-43)
SCALE = 6463.81735715902


def get_file_list(directory):
    """Full paths of the folder's ``.npz`` records in the order of their file names (= of their start times)."""
    names = sorted(name for name in os.listdir(directory) if name.endswith(".npz"))
    return [os.path.join(directory, name) for name in names]


def get_time_from_file_path(file_path, time_format="%Y%m%d_%H%M%S"):
    """The record's start time: the file name up to its first dot, read with ``time_format``."""
    stamp = os.path.basename(file_path).partition(".")[0]
    return datetime.strptime(stamp, time_format)


class _Pending:
    """A record read and upload in flight (the background thread's future)."""

    def __init__(self, fut):
        self._fut = fut

    def __call__(self, device):
        t, x_axis, t_axis, scale, ev = self._fut.result()
        cur = torch.cuda.current_stream(device)
        cur.wait_event(ev)
        t.record_stream(cur)  # allocated on the side stream, used on the caller's
        return t, x_axis, t_axis, scale

    def drain(self):
        try:
            ev = self._fut.result()[4]
        except Exception:  # the read's own error belongs to whoever uses the record
            return
        ev.synchronize()


class ImagingIO:
    def __init__(self, directory, root, ch1=400, ch2=540, smoothing=True, device=None, prefetch=1):
        """The records of ``root/directory``; ch1 / ch2: the channel cut of every record; smoothing: whether
        savgol_filter(21, 15) is applied; device / prefetch: see the module docstring.  Nothing here touches the device."""
        self.data_files = get_file_list(os.path.join(root, directory))
        self.ch1, self.ch2 = ch1, ch2
        self.smoothing = smoothing
        self.device = device
        self.prefetch = int(prefetch)
        self._stage = None

    def get_time_interval(self):
        """Seconds from the first record's start to the second's (the folder's records are evenly spaced)."""
        stamps = [get_time_from_file_path(f) for f in self.data_files[:2]]
        return (stamps[1] - stamps[0]).total_seconds()  # IndexError for a folder of fewer than two records

    def __contains__(self, item):
        return 0 < item < len(self.data_files)  # the reference's test: index 0 is not "in"

    def __len__(self):
        return len(self.data_files)

    def close(self):
        """Drain and stop the prefetch thread (also done when the object is collected)."""
        st, self._stage = self._stage, None
        if st is not None:
            st["pool"].shutdown(wait=True)
            st["stream"].synchronize()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # ------------------------------------------------------------------ host side
    def _read(self, idx):
        """(host record float32 / float64 C-contiguous, x_axis, t_axis, scale) of file idx."""
        file_path = self.data_files[idx]  # IndexError past the end: what ends `for ... in imagingIO`
        data, x_axis, t_axis = _read_das_npz(file_path, ch1=self.ch1, ch2=self.ch2)
        folder = file_path.split("/")[-2]  # the date folder's name, compared as a string
        scale = SCALE if folder > SCALE_AFTER_DATE else 1
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)
        return np.ascontiguousarray(data), x_axis, t_axis, scale

    def _device(self):
        if self.device is None:
            from ..device import default_device
            self.device = default_device()
        return torch.device(self.device)

    # ------------------------------------------------------------------ device side
    def _finish(self, t, scale):
        from .. import _lib
        from ..preprocess import savgol_smooth
        if self.smoothing:
            return savgol_smooth(t, 21, 15, divisor=float(scale))
        if scale != 1 and t.numel():
            _lib.call("dvh_divide_rows", _lib.ptr(t), 0 if t.dtype == torch.float32 else 1, t.shape[0], t.stride(0),
                      t.shape[1], float(scale), _lib.stream_of(t.device))
        return t

    def __getitem__(self, idx):
        host, x_axis, t_axis, scale = self._read(idx)
        t = torch.from_numpy(host).to(self._device())
        return self._finish(t, scale), x_axis, t_axis

    def _staging(self, dev):
        if self._stage is None:
            self._stage = dict(stream=torch.cuda.Stream(device=dev), pool=cf.ThreadPoolExecutor(1),
                               pinned=[None, None], free=[None, None])
        return self._stage

    def _upload(self, idx, dev):
        """Background thread: read file idx, copy it into pinned buffer idx & 1 and send it on the side stream."""
        st = self._staging(dev)
        host, x_axis, t_axis, scale = self._read(idx)
        b = idx & 1
        if st["free"][b] is not None:
            st["free"][b].synchronize()  # the copy that last read this pinned buffer is done
        if st["pinned"][b] is None or st["pinned"][b].numel() < host.nbytes:
            with torch.cuda.device(dev):  # pinned through the record's device, not this thread's current one
                st["pinned"][b] = torch.empty(max(host.nbytes, 16), dtype=torch.uint8, pin_memory=True)
        pin = st["pinned"][b][:host.nbytes].view(torch.from_numpy(host).dtype).view(host.shape)
        np.copyto(pin.numpy(), host)
        with torch.cuda.stream(st["stream"]):
            t = torch.empty(host.shape, dtype=pin.dtype, device=dev)
            t.copy_(pin, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st["stream"])
        st["free"][b] = ev
        return t, x_axis, t_axis, scale, ev

    def __iter__(self):
        n = len(self.data_files)
        if self.prefetch <= 0 or n == 0:
            for k in range(n):
                yield self[k]
            return
        dev = self._device()
        pool = self._staging(dev)["pool"]
        pending = _Pending(pool.submit(self._upload, 0, dev))
        try:
            for k in range(n):
                cur, pending = pending, None
                t, x_axis, t_axis, scale = cur(dev)
                if k + 1 < n:
                    pending = _Pending(pool.submit(self._upload, k + 1, dev))
                yield self._finish(t, scale), x_axis, t_axis
        finally:
            if pending is not None:  # an abandoned read: its copy must not outlive the loop
                pending.drain()
