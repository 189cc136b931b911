"""Diagnostic: per-phase, per-wave timeline of sr_tail_train_kernel (tail forward + loss + backward) from in-kernel stamps.
Needs the diagnostic library: python -m mobilesuperresolution_amd.build --debug; run with SR_HOTPATH_DEBUG_LIB=1
(or SR_HOTPATH_LIB_PATH=<another diagnostic build of the same sources> for an A/B of kernel variants).
    SR_HOTPATH_DEBUG_LIB=1 python tools/stamp_tail.py [batch] [features] [loss kind] [workgroups]"""
import os, sys
os.environ.setdefault("SR_HOTPATH_DEBUG_LIB", "1")
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobilesuperresolution_amd import _lib as L, hotpath as HP
n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
f = int(sys.argv[2]) if len(sys.argv) > 2 else 24
kind = int(sys.argv[3]) if len(sys.argv) > 3 else 1
wgs = int(sys.argv[4]) if len(sys.argv) > 4 else 256
h = w = 48
dev = torch.device("cuda", 0)
tb = HP.ends_tables(f, 4, dev)
g = torch.Generator().manual_seed(1)
src_tail = (torch.randn(tb["tail_size"], generator=g) * 0.05).cuda()
src_tail[-2], src_tail[-1] = 0.0, 1.0
blob = HP.pack_tail(src_tail, f, 4, torch.bfloat16)
feat = torch.randn(n, h, w, f, generator=g).cuda().bfloat16()
x = torch.rand(n, 3, h, w, generator=g).cuda()
hr = torch.rand(n, 3, 4 * h, 4 * w, generator=g).cuda()
dfeat = torch.empty_like(feat)
part = torch.zeros(wgs, tb["tail_slab"], device=dev)
lpart = torch.zeros(wgs, device=dev)
st = torch.zeros(wgs * 16 * 16 * 2, dtype=torch.int64, device="cuda")
lib = L.lib()
def run():
    L.check(lib.sr_tail_train(hr.data_ptr(), kind, 1.0 / hr.numel(), lpart.data_ptr(), feat.data_ptr(), x.data_ptr(), 0.5, blob.data_ptr(),
                              dfeat.data_ptr(), part.data_ptr(), wgs, n, h, w, f, 4, 1, L.stream_ptr()), "tail_train")
for it in range(5):
    run()
torch.cuda.synchronize()
L.check(lib.sr_debug_set_stamps(st.data_ptr(), wgs), "set")
for it in range(3):
    run()
torch.cuda.synchronize()
L.check(lib.sr_debug_set_stamps(None, 0), "unset")
raw = st.cpu().numpy().reshape(wgs, 16, 16, 2).astype(np.float64)
s = raw[..., 0] * 10.0                                                    # ns (100 MHz)
cyc = raw[..., 1]
tiles = n * ((h + 11) // 12) * ((w + 23) // 24)
busy = min(wgs, tiles)                                                    # workgroups past the tile count only write zeros
nw = 14
names = ["stage + barrier", "forward products", "HR read, dconv + terms, barriers", "loss sums + dfeat", "weight-gradient products",
         "slab + loss_part"]
nst = len(names) + 1
if tiles > wgs:
    print("more tiles than workgroups: the stamps below are those of each workgroup's FIRST tile (and the last phase is not its end)")
s, cyc = s[:busy, :nw, :nst], cyc[:busy, :nw, :nst]
t0 = s[..., 0].min()
print(f"sr_tail_train_kernel batch {n}, {h}x{w}, F {f}, loss {kind}: {busy} workgroups with a tile, {nw} waves, {nst} stamps; "
      f"first start -> last end {s[..., nst - 1].max() - t0:.0f} ns")
print("workgroup start spread %.0f ns" % (s[:, 0, 0].max() - t0))
for k in range(nst - 1):
    d = s[..., k + 1] - s[..., k]
    dcy = cyc[..., k + 1] - cyc[..., k]
    # a phase ends for the workgroup when its slowest wave is through: the max over waves is what the chain pays
    wg = s[..., k + 1].max(axis=1) - s[..., k].max(axis=1)
    print("%-34s median %6.0f ns = %6.0f cycles  p10 %6.0f  p90 %6.0f  slowest-wave to slowest-wave %6.0f   per-wave median ns: %s" % (
          names[k], np.median(d), np.median(dcy), np.percentile(d, 10), np.percentile(d, 90), np.median(wg),
          " ".join("%5.0f" % v for v in np.median(d, axis=0))))
dt = s[..., nst - 1] - s[..., 0]
dc = cyc[..., nst - 1] - cyc[..., 0]
print("shader clock over the kernel: median %.2f GHz" % np.median(dc / np.maximum(dt, 1)))
tot = s[..., nst - 1].max(axis=1) - s[..., 0].min(axis=1)
print("per-WG total median %.0f ns  p10 %.0f  p90 %.0f" % (np.median(tot), np.percentile(tot, 10), np.percentile(tot, 90)))
