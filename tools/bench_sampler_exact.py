"""The conditioned sampler with the reference's API default exact_grad=True (src/thor/score.py:44: the likelihood score differentiates
through the network) next to exact_grad=False (what the shipped experiment configs use): ms per sampler step, window evaluations/s and
peak memory at F = 4, k = 6, 128x128, bf16, window batch 128, for three legs in ONE process, alternated round by round:
  noexact   exact_grad=False (the fused guidance kernel)
  exact     exact_grad=True on the autograd route (every window taped, one backward at the end)
  streamed  exact_grad=True window by window (score_fn.py::_guided_exact_streamed)
Environment: L (121), LEGS (comma list, default all three -- at L = 8737 only ``streamed`` and ``noexact`` fit the device), STEPS (4 sampler
steps per timed round), ROUNDS (3), FROZEN (1).  Also prints the vendor library's dense bf16 GEMM rate on this chip in this run, and how far
the streamed result is from the autograd route's when both ran."""
import contextlib, io, os, sys, time
sys.path.insert(0, os.getcwd())
import torch
import bench
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.score_fn import BatchedScoreFunction, PoolStrideOperator

dev = torch.device("cuda:0")
F, k, H, L = 4, 6, 128, int(os.environ.get("L", "121"))
LEGS = [s for s in os.environ.get("LEGS", "noexact,exact,streamed").split(",") if s]
STEPS, ROUNDS = int(os.environ.get("STEPS", "4")), int(os.environ.get("ROUNDS", "3"))
w = 2 * k + 1
torch.manual_seed(0)
net = ScoreUNet(channels=F * w, spatial=2, activation=torch.nn.SiLU, **bench.DEFAULT_CFG).to(dev).eval()
net.precision = "bf16"
if os.environ.get("FROZEN", "1") == "1":
    net.requires_grad_(False)  # the sampler's copy in the reference: a pickled snapshot saved with requires_grad_(False) (training_loop.py:253-265)
pipe = SDAPipeline()
A = PoolStrideOperator(16, 6)
std = torch.tensor([0.1692666615037876, 0.0425178630338289, 0.3268027589410125, 0.3268027589410125]).view(1, F, 1, 1)
g = torch.Generator(device=dev).manual_seed(L)
truth = torch.randn((L, F, H, H), device=dev, generator=g) * 0.5 + 0.5
noise = torch.randn((L, F, H, H), device=dev, generator=g)
y = A(truth)
del truth


def vendor_gemm_tflops(n=8192):
    ga, gb = torch.randn(n, n, device=dev).bfloat16(), torch.randn(n, n, device=dev).bfloat16()
    for _ in range(3):
        torch.matmul(ga, gb)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        torch.matmul(ga, gb)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * n ** 3 / (e0.elapsed_time(e1) / 20 * 1e-3) / 1e12


sfs = {}
for leg in LEGS:
    with contextlib.redirect_stdout(io.StringIO()):
        sf = BatchedScoreFunction(net, markov_order=k, batch_size=128, device=dev, noise_process=pipe)
        sf.condition_on(A=A, y=y, std=std, gamma=0.0007196856730011522, exact_grad=leg != "noexact")
        sf.exact_streamed = {"noexact": None, "exact": False, "streamed": True}[leg]
    sfs[leg] = sf


def run(leg, steps):
    with contextlib.redirect_stdout(io.StringIO()):
        x = pipe.sample(sfs[leg], noise, steps=steps, corrections=0, device=dev, show_progressbar=False)
    torch.cuda.synchronize()
    return x


times, peak, finite = {leg: [] for leg in LEGS}, {}, {}
for leg in LEGS:  # warm-up of every shape, and the peak memory of one step on a clean allocator
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    finite[leg] = bool(torch.isfinite(run(leg, 1)).all())
    peak[leg] = torch.cuda.max_memory_allocated()
for r in range(ROUNDS):  # alternate the legs: what shares the host shares it with all of them
    for leg in LEGS:
        t0 = time.perf_counter()
        run(leg, STEPS)
        times[leg].append((time.perf_counter() - t0) / STEPS)
print(f"vendor GEMM (torch.matmul 8192^3 bf16, this run): {vendor_gemm_tflops():.0f} TFLOP/s", flush=True)
for leg in LEGS:
    ts = sorted(times[leg])
    if not ts:
        print(f"L = {L} {leg:8s}: warm-up step only, peak memory {peak[leg] / 2**30:7.2f} GiB, finite {finite[leg]}", flush=True)
        continue
    med = ts[len(ts) // 2]
    print(f"L = {L} frozen = {os.environ.get('FROZEN', '1')} {leg:8s}: {1e3 * med:9.2f} ms per sampler step (median of {len(ts)} rounds of {STEPS}; "
          f"min {1e3 * ts[0]:.2f}, max {1e3 * ts[-1]:.2f}), {(L - w + 1) / med:9.1f} window evaluations/s, peak memory {peak[leg] / 2**30:7.2f} GiB, "
          f"finite {finite[leg]}", flush=True)
if "exact" in sfs and "streamed" in sfs:
    t = torch.tensor(0.6)
    a, b = sfs["exact"](noise, t).clone(), sfs["streamed"](noise, t).clone()
    print(f"one evaluation at t = 0.6, streamed vs autograd route: max |diff| / max |ref| = {(a - b).abs().max().item() / a.abs().max().item():.3e}",
          flush=True)
