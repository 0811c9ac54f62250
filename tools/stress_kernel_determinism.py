#!/usr/bin/env python3
"""Is every launch of the round-6 conv kernels bit-identical to the first one?  Repeats small launches (the shapes of
tests/test_gpu_host.py::test_bf16_and_fp16_training_track_fp32_training and a few more) N times, alone and beside a memory-bound kernel on
another stream that perturbs the timing of the LDS-DMA, and counts the launches whose output differs in any bit from the first.
A kernel with a timing-dependent LDS race shows up here; summation order cannot (one launch = one fixed order).
    python tools/stress_kernel_determinism.py [N]"""
import math, os, sys
sys.path.insert(0, os.getcwd())
os.environ.setdefault("C2W_CONV_S2_PATCH", "1")  # the stride-2 forward kernel is off by default (csrc/knobs.h); this tool is about it
import torch
from climate2weather_amd import ops, _lib

N = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
dev = torch.device("cuda:0")
S1, S2, TS2 = ops.CONV_S1, ops.CONV_S2, ops.CONV_TS2
NAMES = {0: "gather", 1: "8x16", 2: "16x16", 3: "pair", 4: "ts2", 5: "s2"}
CASES = [("S2 fwd 64->128 32^2->16^2 (one K chunk)", S2, 8, 32, 64, 128), ("S2 fwd 128->128 32^2->16^2 (two K chunks)", S2, 8, 32, 128, 128),
         ("S2 fwd 256->128 32^2->16^2 (four K chunks)", S2, 8, 32, 256, 128), ("S2 fwd 128->128 16^2->8^2 (two images per tile)", S2, 8, 16, 128, 128),
         ("S1 64->64 @32^2 (one chunk, second patch buffer idle)", S1, 8, 32, 64, 64), ("S1 128->128 @16^2 (two chunks)", S1, 8, 16, 128, 128),
         ("S1 256->256 @16^2 (four chunks)", S1, 8, 16, 256, 256), ("S1 128->128 @8^2 (pairs)", S1, 8, 8, 128, 128),
         ("S1 512->512 @8^2 (pairs, eight chunks)", S1, 32, 8, 512, 512), ("S1 64->64 @32^2, 512 workgroups (one patch buffer)", S1, 64, 32, 64, 64),
         ("TS2 128->64 16^2->32^2 (two classes per workgroup)", TS2, 8, 16, 128, 64)]
side = torch.cuda.Stream()
big = torch.empty(64 << 20, dtype=torch.float32, device=dev)
for dt, td in ((_lib.DTYPE_BF16, torch.bfloat16), (_lib.DTYPE_F16, torch.float16)):
    for name, mode, B, Hin, Cin, Cout in CASES:
        Hout = Hin // 2 if mode == S2 else (2 * Hin if mode == TS2 else Hin)
        g = dict(B=B, Hin=Hin, Win=Hin, Cin=Cin, Hout=Hout, Wout=Hout, Cout=Cout, ldy=Cout, wrows=Cout, mode=mode)
        # TWO operand sets, alternating: a launch that reads an LDS slot before its own LDS-DMA has landed would otherwise find the previous
        # launch's identical bytes there and pass
        sets = []
        for seed in (1, 2):
            torch.manual_seed(seed)
            x = torch.randn(B * Hin * Hin, Cin, device=dev).to(td)
            w = (torch.randn(Cout, 9, Cin, device=dev) / math.sqrt(9 * Cin)).to(td)
            bias = torch.randn(Cout, device=dev)
            res = torch.randn(B * Hout * Hout, Cout, device=dev).to(td)
            kw = dict(res=res) if mode == TS2 else {}
            y0 = torch.empty(B * Hout * Hout, Cout, dtype=td, device=dev)
            ops.conv(x, w, None if mode == TS2 else bias, y0, g, dt, **kw)
            sets.append((x, w, bias, kw, y0))
        torch.cuda.synchronize()
        bad = torch.zeros(2, dtype=torch.int64, device=dev)
        for phase in (0, 1):
            for i in range(N):
                if phase == 1 and i % 8 == 0:
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        big.mul_(1.0001)
                x, w, bias, kw, y0 = sets[i & 1]
                y = torch.full_like(y0, 3.0)
                ops.conv(x, w, None if mode == TS2 else bias, y, g, dt, **kw)
                bad[phase] += (y.view(torch.int16) != y0.view(torch.int16)).any().to(torch.int64)
            torch.cuda.synchronize()
        print(f"{'bf16' if dt == _lib.DTYPE_BF16 else 'fp16'} {name:70s} kernel {NAMES[ops.conv_dispatch(g, dt)]:6s}: launches differing from the first, of {N}: alone {int(bad[0])}, beside a stream {int(bad[1])}", flush=True)
