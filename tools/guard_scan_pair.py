#!/usr/bin/env python
"""GPU dev tool: iaf_nonfinite_scan and iaf_nonfinite_scan_sumsq, 60 launches each in alternation, on one buffer of N floats (default:
the flat gradient of the BASELINE geometry, 41557932) -- a short program for  rocprofv3 --kernel-trace --stats -- python
tools/guard_scan_pair.py [N], whose per-kernel averages compare the two scans without launch gaps or event overhead."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from iaf_amd import _capi

n = int(sys.argv[1]) if len(sys.argv) > 1 else 41557932
lib = _capi.lib()
g = torch.Generator(device="cuda").manual_seed(1)
buf = torch.randn(n, device="cuda", generator=g) * 1e-2
status = torch.zeros(2, device="cuda")
guard = torch.zeros(4, dtype=torch.int32, device="cuda")
partials = torch.zeros(2048, dtype=torch.float64, device="cuda")
sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
P = lambda t: ctypes.c_void_p(t.data_ptr())
st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
for _ in range(60):
    _capi.check(lib.iaf_nonfinite_scan(P(buf), n, P(status), 1, P(guard), st()))
    _capi.check(lib.iaf_nonfinite_scan_sumsq(P(buf), n, P(status), 1, P(guard), P(partials), P(sumsq), st()))
torch.cuda.synchronize()
print("n", n, "guard", guard.tolist(), "sumsq", float(sumsq.item()), "ref", float((buf.double() ** 2).sum().item()))
