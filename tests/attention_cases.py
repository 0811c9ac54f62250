"""Shared cases of the attention bound tests (CPU tier and GPU tier): the route rule, the seeded input regimes, the planted defects
and the two bound checks.  The references and the error model are in fp64_ref.py; nothing here calls climate2weather_amd.ops."""
import math

import torch
import torch.nn.functional as F

import emu_ops as E
import fp64_ref as R

F32, BF16, F16 = E.DTYPE_F32, E.DTYPE_BF16, E.DTYPE_F16
SECTION = {"q": 0, "k": 1, "v": 2}


def attn_route(B, T, C, dt, valu_knob=False):
    """the library's eligibility rule (attention_mfma.hip:469-471, 518-520), restated"""
    ok16 = dt in (BF16, F16) and C % 32 == 0 and C <= 512 and B > 0 and not valu_knob
    if ok16 and T == 64:
        return R.T64
    if ok16 and T > 64 and T % 64 == 0 and T <= 4096:
        return R.BLOCKS
    return R.VALU


def sect(ref, s, C):
    i = SECTION[s]
    return R.V(ref.v[:, i * C:(i + 1) * C], ref.e[:, i * C:(i + 1) * C])


def forward_bounds(qkv, o, lse, B, T, C, dt, route, tag, parts=None):
    ro, rl = R.attention_forward(qkv, B, T, C, dt, route, parts=parts)
    wo = R.assert_within(o, ro, what=f"{tag} o", layout=R.attn_layout(B, T, C, "o"))
    wl = R.assert_within(lse, rl, what=f"{tag} lse", layout=R.attn_layout(B, T, C, ()))
    R.report(f"{tag} forward o", wo)
    R.report(f"{tag} forward lse", wl)
    return ro, rl


def backward_bounds(qkv, o_in, do, lse_in, dqkv, delta, B, T, C, dt, route, tag, parts=None):
    """dq, dk, dv each within their own bound; delta_ws within rowdot's where the route fills it (VALU, BLOCKS)"""
    rg = R.attention_backward(qkv, o_in, do, lse_in, B, T, C, dt, route, parts=parts)
    for s, i in SECTION.items():
        w = R.assert_within(dqkv[:, i * C:(i + 1) * C], sect(rg, s, C), what=f"{tag} d{s}", layout=R.attn_layout(B, T, C, s))
        R.report(f"{tag} d{s}", w)
    if route != R.T64 and delta is not None:
        R.report(f"{tag} delta", R.assert_within(delta, R.rowdot(do, o_in, B * T, C), what=f"{tag} delta", layout=R.attn_layout(B, T, C, ())))
    return rg


REGIMES = ("randn", "peaked", "shifted", "rising", "falling", "uniform", "smallgrad")


def attention_inputs(regime, B, T, C, dtype, seed=1):
    """seeded (qkv rows (B * T, 3 C), do rows (B * T, C)) of the storage type, on the CPU.  Regimes:
      randn      randn * 1.5, do = randn (the parity tests' inputs)
      peaked     q, k = randn * 3.5: scores of standard deviation 12, near one-hot rows
      shifted    q, k = noise * 1.2 orthogonal to u, plus the same u on every row, |u|^2 C^-1/2 = 45: |lse| about 50, softmax as spread as randn * 1.2
      rising     q = randn * 0.7 + a w, k of key group b = randn * 0.7 + b a w (w = the unit diagonal, a^2 C^-1/2 = 4): every group of
                 attention_group(T) keys raises the scores by 4;   falling: the mirror image, group 0 holds the maximum
      uniform    all k rows of an image identical (P = 1 / T, dq = 0 in exact arithmetic)
      smallgrad  randn with do * 2^-12 (fp16: dS and the gradients are subnormal)"""
    T_ = R._T(dtype)
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn((B, T, C), generator=g, dtype=R.D) for _ in range(4))
    v = v * 1.5
    if regime in ("randn", "smallgrad", "uniform"):
        q, k = q * 1.5, k * 1.5
        if regime == "uniform":
            k = k[:, :1].expand(B, T, C)
        if regime == "smallgrad":
            do = do * 2.0 ** -12
    elif regime == "peaked":
        q, k = q * 3.5, k * 3.5
    elif regime == "shifted":
        u = (torch.randint(0, 2, (C,), generator=g).to(R.D) * 2 - 1) * math.sqrt(45.0 / math.sqrt(C))
        uh = u / u.norm()
        q, k = ((n - (n @ uh).unsqueeze(-1) * uh) * 1.2 + u for n in (q, k))
    elif regime in ("rising", "falling"):
        grp = attention_group(T)
        a = 2.0 * C ** 0.25
        b = torch.arange(T) // grp
        if regime == "falling":
            b = b.max() - b
        w = torch.full((C,), 1.0 / math.sqrt(C), dtype=R.D)
        q = q * 0.7 + a * w
        k = k * 0.7 + (a * b.to(R.D)).view(1, T, 1) * w
    else:
        raise ValueError(regime)
    return torch.cat((q, k, v), -1).reshape(B * T, 3 * C).to(T_), do.reshape(B * T, C).to(T_)


def attention_group(T):
    """the key group of the rising / falling regimes: the kernels' 64-key block where there is more than one, else a 16-row strip"""
    return R.KB if T > R.KB and T % R.KB == 0 else 16


def attention_regime_stats(qkv, B, T, C):
    """(mean row maximum of P, min |lse|, max |lse|, mean number of key groups after the first that raise the row maximum,
    mean number of groups after the first that do not)"""
    x = R.attention_exact(qkv, B, T, C)
    grp = attention_group(T)
    ng = -(-T // grp)
    S = F.pad(x["S"], (0, ng * grp - T), value=-math.inf).view(B, T, ng, grp).amax(-1)
    run = S.cummax(-1).values
    up = (run[..., 1:] > run[..., :-1]).to(R.D).sum(-1).mean().item()
    return x["P"].amax(-1).mean().item(), x["lse"].abs().min().item(), x["lse"].abs().max().item(), up, ng - 1 - up


def attention_defect(kind, qkv, do, B, T, C, image=0):
    """A planted defect of the attention kernels as (section, fp64 term, where): rows (B * T, C) to ADD to the kernel's o / dq / dk / dv.
    Each is placed where it carries weight (the strip / tile / key with the largest share), never on a zero-weight key.
      p_tile     one 16 x 16 tile of P missing from o: the strip and key tile with the largest summed weight
      key        the single key with the largest weight summed over one 16-row strip dropped from that strip's o
      alpha      BLOCKS: at the transition where the row maximum grows most (summed over the image) the accumulated earlier blocks are
                 not multiplied by alpha = exp(m_old - m_new): they stay (1 / alpha - 1) too large
      dq_block   BLOCKS: the key block with the largest |dS| missing from dq
      delta_row  delta of row i taken from row i + 1 (the last row from the one before) in dq, on the strip where |delta_i - delta_i+1| P |k| is largest
      ds_scale   dS without the s^2 factor on one 16 x 16 tile (the largest |dS| tile) of dk"""
    x = R.attention_exact(qkv, B, T, C, do)
    P, v, k, q, s2 = x["P"][image], x["v"][image], x["k"][image], x["q"][image], x["s2"]
    out = torch.zeros((B, T, C), dtype=R.D, device=P.device)
    ns, nt = -(-T // 16), -(-T // 16)
    pad = ns * 16 - T

    def tiles(Wm):  # (ns, nt) sums of a (T, T) matrix over 16 x 16 tiles
        return F.pad(Wm, (0, pad, 0, pad)).view(ns, 16, nt, 16).sum((1, 3))

    if kind == "p_tile":
        i = int(tiles(P).argmax())
        st, kt = divmod(i, nt)
        r, c = slice(16 * st, min(16 * st + 16, T)), slice(16 * kt, min(16 * kt + 16, T))
        out[image, r] = -P[r, c] @ v[c]
        return "o", out.view(B * T, C), f"strip {st}, key tile {kt}"
    if kind == "key":
        w = F.pad(P, (0, 0, 0, pad)).view(ns, 16, T).sum(1)
        st, j = divmod(int(w.argmax()), T)
        r = slice(16 * st, min(16 * st + 16, T))
        out[image, r] = -P[r, j:j + 1] * v[j:j + 1]
        return "o", out.view(B * T, C), f"strip {st}, key {j}"
    if kind == "alpha":
        M, _ = R._running_max(x["S"][image:image + 1], T)
        rise = (M[0, :, 1:] - M[0, :, :-1])  # (T, nb - 1) >= 0
        t = int(rise.sum(0).argmax()) + 1
        early = P[:, : R.KB * t] @ v[: R.KB * t]
        out[image] = (rise[:, t - 1].clamp_max(60.0).exp() - 1).unsqueeze(-1) * early
        return "o", out.view(B * T, C), f"transition into key block {t}"
    dS = x["dS"][image]
    if kind == "dq_block":
        nb = T // R.KB
        jb = int(dS.abs().view(T, nb, R.KB).sum((0, 2)).argmax())
        c = slice(R.KB * jb, R.KB * jb + R.KB)
        out[image] = -s2 * dS[:, c] @ k[c]
        return "q", out.view(B * T, C), f"key block {jb}"
    if kind == "delta_row":
        dl = x["delta"][image]
        nxt = torch.cat((dl[1:], dl[-2:-1])) if T > 1 else dl
        full = s2 * (dl - nxt).unsqueeze(-1) * (P @ k)  # P (dP - delta') - P (dP - delta) = P (delta - delta')
        st = int(F.pad(full.abs().sum(-1), (0, pad)).view(ns, 16).sum(1).argmax())
        r = slice(16 * st, min(16 * st + 16, T))
        out[image, r] = full[r]
        return "q", out.view(B * T, C), f"strip {st}"
    if kind == "ds_scale":
        i = int(tiles(dS.abs()).argmax())
        st, kt = divmod(i, nt)
        r, c = slice(16 * st, min(16 * st + 16, T)), slice(16 * kt, min(16 * kt + 16, T))
        out[image, c] = (1 - s2) * dS[r, c].t() @ q[r]
        return "k", out.view(B * T, C), f"query strip {st}, key tile {kt}"
    raise ValueError(kind)


def stale_upper_half(dqkv, B, T, C, section, image=1):
    """defect (e): the upper wave half's column tiles (channels >= (C / 16) / 2 * 16) of one section of one image (B >= 2) left at the
    previous content -- the previous image's values of the same section: what an earlier launch over a smaller batch would have left
    there, of the right size and distribution, so a check of the tensor's scale alone does not see it by construction (and not
    the same image's other rows: with identical keys all rows of dv are equal)"""
    bad = dqkv.to(R.D).clone().view(B, T, -1)
    s = "qkv".index(section) if bad.shape[-1] == 3 * C else 0
    cols = slice(s * C + (C // 16) // 2 * 16, (s + 1) * C)
    bad[image, :, cols] = bad[image - 1, :, cols]
    return bad.view(B * T, -1)
