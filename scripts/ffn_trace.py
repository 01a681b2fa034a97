"""Summarise phase traces of the decode FFN launches (development).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -DLLMI_LAYER_TRACE \
          scripts/gemv_sweep.hip -o scripts/gemv_sweep
    LLMI_FFN_TRACE_DIR=dir scripts/gemv_sweep 200 4b.gate_up      (and 4b.down)
    python scripts/ffn_trace.py dir/4b.gate_up.gelu_late.bin dir/4b.gate_up.gelu.bin ...

Each file holds one launch (the last of 24 back to back, every one reading another copy of the weight from HBM):
[work-group][16] 64-bit words, layer_body.h LAYER_MARK -- wall clocks (100 MHz) of
  0 start, 1 first weight passes issued, 2 prologue operands landed (down: x quantized), 3 x complete in LDS,
  4 last weight pass issued, 5 last pass consumed, 6 epilogue stores issued, 7 end,
  8 / 9 the prologue's first / second reduction done (gate_up only); word 10 HW_ID, word 11 XCC_ID of wave 0.
The FFN launches read no position-dependent operand: the trace at position 537 is the trace at any position.
Times are us from the first work-group's start; stamps are thread 0's (wave 0 of each work-group).
"""
import sys

import numpy as np

W = 16
PHASES = [(0, "start"), (1, "first passes issued"), (2, "prologue operands landed"), (8, "first reduction done"),
          (9, "second reduction done"), (3, "x complete (barrier)"), (4, "last pass issued"), (5, "last pass consumed"),
          (6, "epilogue stores issued"), (7, "end")]


def summarise(path):
    raw = np.fromfile(path, dtype=np.uint64).reshape(-1, W)
    raw = raw[raw[:, 0] > 0]
    t = raw[:, :10].astype(np.float64)
    t0 = t[:, 0].min()
    rel = np.where(t > 0, (t - t0) / 100.0, np.nan)
    hw, xcc = raw[:, 10].astype(np.int64), raw[:, 11].astype(np.int64) & 0xF
    # HW_ID: cu_id [11:8], sh_id [12], se_id [15:13]
    cu = (xcc << 8) | ((hw >> 8) & 0xFF)
    n_per_cu = np.unique(cu, return_counts=True)[1]
    print(f"{path}: {len(raw)} work-groups")
    print(f"  {'phase':26s} {'mean':>7s} {'max':>7s}   (us from the first start)")
    for k, name in PHASES:
        if np.isfinite(rel[:, k]).any():
            print(f"  {name:26s} {np.nanmean(rel[:, k]):7.2f} {np.nanmax(rel[:, k]):7.2f}")
    dur = rel[:, 7] - rel[:, 0]
    print(f"  work-group start -> end    {dur.mean():7.2f} {dur.max():7.2f}")
    for a, b, name in ((0, 1, "issue of the first passes"), (3, 4, "x complete -> last issued"),
                       (4, 5, "last issued -> consumed"), (5, 7, "consumed -> end")):
        d = rel[:, b] - rel[:, a]
        if np.isfinite(d).any():
            print(f"  {name:26s} {np.nanmean(d):7.2f} {np.nanmax(d):7.2f}")
    end = rel[:, 7]
    print(f"  first start -> last end: {end.max():.2f} us; start spread {rel[:, 0].max():.2f} us; "
          f"end spread {end.max() - end.min():.2f} us (std {end.std():.2f})")
    per = []
    for x in sorted(set(xcc.tolist())):
        e = end[xcc == x]
        per.append(f"xcd{x}: n {len(e)} last {e.max():.2f} spread {e.max() - e.min():.2f}")
    print("  per XCD end times -- " + "; ".join(per))
    n_cu = 256
    print(f"  CUs used {len(n_per_cu)}; with 2 or more work-groups {int((n_per_cu >= 2).sum())}; "
          f"with none (of {n_cu}) {n_cu - len(n_per_cu)}")


for p in sys.argv[1:]:
    summarise(p)
