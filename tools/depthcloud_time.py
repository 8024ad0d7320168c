"""Host wall time of rsreg_cloud_from_depth (depth + colour image -> organized cloud in HBM: 5 bytes a pixel over the link) on
rendered frames of 50 k, 307 k and 1 M pixels -- z quantized at depth_scale 0.001 plus a colour image of the same size -- the
first call and the best of the repeats, as the call returns (the images have arrived, the kernel is queued) and with the
context synchronized behind it (the cloud is complete).  Beside it, in the same run: rsreg_cloud_upload of the same frame's
32-byte records (complete when it returns), and the kernel's own time from HIP events around rsreg_cloud_from_depth_device
with the images already in HBM.  The claim to check: the call approaches 5/32 of the upload's time where the link dominates.

    python tools/depthcloud_time.py [--sizes 50k,N300,N1M] [--repeats 20] [--out profiles/depthcloud_time.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api, lib as L, synth  # noqa: E402


def images(cloud):
    """what a camera would have delivered for this rendered frame: depth in mm, colour in b, g, r order, its pinhole"""
    w, h = cloud.width, cloud.height
    depth = np.rint(cloud.points["z"].astype(np.float64) * 1000.0).astype(np.uint16).reshape(h, w)
    rgba = cloud.points["rgba"].reshape(h, w)
    color = np.stack([rgba & 0xff, (rgba >> 8) & 0xff, (rgba >> 16) & 0xff], axis=2).astype(np.uint8)
    f = 385.0 * (w / 640.0)
    cam = dict(width=w, height=h, ppx=w / 2.0, ppy=h / 2.0, fx=f, fy=f)
    return depth, color, api.depth_params(w, h, depth=cam, color=cam)


def timed(fn, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:])


class Hip:
    """the few HIP runtime calls the kernel's timing needs, from the runtime librsreg.so itself runs on"""

    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")

    def ok(self, rc):
        if rc:
            raise RuntimeError("HIP error %d" % rc)

    def stream(self):
        s = C.c_void_p()
        self.ok(self.rt.hipStreamCreate(C.byref(s)))
        return s

    def event(self):
        e = C.c_void_p()
        self.ok(self.rt.hipEventCreate(C.byref(e)))
        return e

    def record(self, e, s):
        self.ok(self.rt.hipEventRecord(e, s))

    def elapsed_ms(self, e0, e1):
        self.ok(self.rt.hipEventSynchronize(e1))
        ms = C.c_float(0)
        self.ok(self.rt.hipEventElapsedTime(C.byref(ms), e0, e1))
        return ms.value


def device_bytes(ctx, buf):
    """the bytes of `buf` in HBM, as 16-byte records of a cloud the caller keeps: (cloud, device address)"""
    raw = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    padded = np.zeros((len(raw) + 15) // 16 * 16, np.uint8)
    padded[: len(raw)] = raw
    c = api.DeviceCloud(ctx=ctx)
    L.check(L.lib().rsreg_cloud_upload(c.h, padded.ctypes.data, len(padded) // 16, 16, len(padded) // 16, 1, 0), ctx.h)
    return c, c.device_ptr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthcloud_time.jsonl"))
    a = ap.parse_args()
    L.lib()
    hip = Hip()
    stream = hip.stream()
    ctx = api.Context(0, stream=stream.value)      # the context runs on a stream this tool can record events on
    e0, e1 = hip.event(), hip.event()
    rows = []
    for size in a.sizes.split(","):
        depth, color, p = images(synth.render_frame(1, size))
        n = depth.size
        built, up = api.DeviceCloud(ctx=ctx), api.DeviceCloud(ctx=ctx)
        call_first, call = timed(lambda: api.DeviceCloud.from_depth(ctx, depth, color, p, out=built), a.repeats)

        def done():
            api.DeviceCloud.from_depth(ctx, depth, color, p, out=built)
            ctx.synchronize()
        _, done_ms = timed(done, a.repeats)
        records = built.download()
        assert (records.width, records.height) == (depth.shape[1], depth.shape[0])
        up_first, up_ms = timed(lambda: up.upload(records), a.repeats)
        assert up.download().points.tobytes() == records.points.tobytes()
        # the kernel alone: the images in HBM, HIP events on the context's stream around the launch
        (d_keep, d_ptr), (c_keep, c_ptr) = device_bytes(ctx, depth), device_bytes(ctx, color)
        ctx.synchronize()
        kernel = []
        for _ in range(1 + a.repeats):
            hip.record(e0, stream)
            L.check(L.lib().rsreg_cloud_from_depth_device(ctx.h, d_ptr, 2 * depth.shape[1], c_ptr, 3 * depth.shape[1], C.byref(p), built.h), ctx.h)
            hip.record(e1, stream)
            kernel.append(hip.elapsed_ms(e0, e1))
        assert built.download().points.tobytes() == records.points.tobytes()
        row = {"size": size, "pixels": n, "image_bytes": 5 * n, "record_bytes": 32 * n,
               "from_depth_first_ms": round(call_first, 3), "from_depth_call_ms": round(call, 3), "from_depth_done_ms": round(done_ms, 3),
               "upload_first_ms": round(up_first, 3), "upload_ms": round(up_ms, 3),
               "done_over_upload": round(done_ms / up_ms, 3), "bytes_ratio": round(5 / 32, 3),
               "kernel_ms": round(min(kernel[1:]), 4), "kernel_gb_per_s": round(37 * n / (min(kernel[1:]) * 1e-3) / 1e9, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        built.close()
        up.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
