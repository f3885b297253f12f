"""The fused multi-tensor Adam / AdamW step (csrc/optim.hip), element by element after each of three steps, against
torch.optim.Adam / AdamW on the CPU with the reference's non-finite zeroing and clip_grad_norm_ in front: parameters,
exp_avg, exp_avg_sq, the gradient buffer the kernel writes back (grad * grad_scale * clip_coef, or zeros), the
per-tensor step counts, the reported total norm and the zero padding between the tensors of the flat buffers.

Tensor sizes straddle the 65 536-element chunk and the float4 body / scalar tail of mt_adam_kernel; one 4-D conv weight
lives in the flat buffer as KRSC, so its torch state is compared through the same permutation.

Bounds. Step counts, untouched (`used` = 0) tensors, the padding and -- whenever the clip coefficient is 1 on both
sides -- the written-back gradient are compared bitwise. p, m, v are not bitwise equal to torch: the device compiler
contracts `v * b2 + (1 - b2) * g * g`, `m + w * (g - m)` and `p + (-step_size) * (m / denom)` (optim.hip:117-120) into
FMAs, torch's CPU kernels round each product (and divide by bias_correction2_sqrt as a multiplication by its
reciprocal). Each of these expressions rounds at most three times on either side (e.g. (1 - b2) * g, * g, the sum), half
an ulp of the larger operand of the final addition each: K_STEP = 3 ulp per step between the two sides, carried from
step to step by the recursion written out in the test. The ulp is taken of the larger of the reference value before and
after the step (and of the gradient for exp_avg), not of the reference value alone: next to a cancellation the
reference value's own ulp says nothing about the rounding of the operands it was formed from. The parameter
additionally inherits the error of exp_avg and exp_avg_sq through its update step_size * m / denom, which can be larger
than the parameter itself; that term is written out where the parameter is checked, and the test asserts that it stays
finite for every element. lr, the betas and the weight decay reach the kernel as doubles, so 1 - beta, the bias
corrections, lr / bias_correction1 and 1 - lr * wd round to fp32 once, as in torch; eps and wd * p use the fp32
values on both sides.
With clipping active the coefficient itself differs: the kernel forms max_norm / (norm + 1e-6) in double from a double
sum of squares and rounds once, torch in fp32 from an fp32 norm of fp32 norms. The distance D (in ulp) between torch's
fp32 coefficient and the float64 formula is measured on the CPU -- the reference's own error -- as a relative number
eps_c, and the gradient is then held to (eps_c + 2^-23) |g| (two product roundings); that error enters the recursion
of exp_avg and exp_avg_sq.
The total norm is accumulated in double here and in fp32 in torch: checked against a float64 norm at 1e-6 relative."""
import math

import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 65535, 65536, 65537, 131075]
CONV = (8, 4, 3, 3)
K_STEP = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _flat_of(t):
    """a reference tensor in the flat buffer's element order (4-D weights: KRSC)"""
    return (t.permute(0, 2, 3, 1) if t.dim() == 4 else t).reshape(-1)


def _ulps(got, ref, scale):
    return ((got.double() - ref.double()).abs() / E.ulp32(scale)).max().item() if got.numel() else 0.0


@pytest.mark.parametrize("clip", [None, 0.05, 1e9], ids=["noclip", "clips", "wide"])
@pytest.mark.parametrize("gscale", [1.0, 0.125], ids=["gs1", "gs8th"])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam_l2"])
def test_fused_adam_elementwise(dev, decoupled, gscale, clip):
    from medvae_disentangled_multimodal_amd.optim import ALIGN, FlatParameters, FusedAdam
    torch.manual_seed(17)
    shapes = [(s,) for s in SIZES] + [CONV]
    wd, betas, lr = (1e-2, (0.9, 0.999), 1e-2) if decoupled else (1e-3, (0.5, 0.999), 1e-2)
    mod = torch.nn.Module()
    ps = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    for i, p in enumerate(ps):
        mod.register_parameter(f"p{i}", p)
    ref = [p.detach().clone().requires_grad_() for p in ps]
    opt_ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ref, lr=lr, betas=betas, weight_decay=wd)
    flat = FlatParameters(mod, dev)
    opt = FusedAdam(flat, lr=lr, betas=betas, weight_decay=wd, decoupled=decoupled, max_grad_norm=clip)
    opt.grad_scale = gscale
    T = len(shapes)
    # the padding between tensors: every flat index no tensor owns
    owned = torch.zeros(flat.numel, dtype=torch.bool)
    for p, off in zip(flat.params, flat.offsets):
        assert off % ALIGN == 0
        owned[off:off + p.numel()] = True
    assert int((~owned).sum()) > 0
    steps_ref = [0] * T
    carry = {}
    for it in range(3):
        grads = [torch.randn(s) * (3.0 if it == 0 else 0.3) for s in shapes]
        if it == 1:
            grads[7][-1] = float("nan")           # the last (scalar-tail) element of the 131 075 tensor
            grads[4][1000] = float("inf")
        dropped = (2, 8) if it == 2 else ()
        used = torch.ones(T, dtype=torch.int32)
        for t in dropped:
            used[t] = 0
        before = [(r.detach().clone(), opt_ref.state[r]["exp_avg"].clone() if r in opt_ref.state and opt_ref.state[r]
                   else torch.zeros_like(r), opt_ref.state[r]["exp_avg_sq"].clone() if r in opt_ref.state and
                   opt_ref.state[r] else torch.zeros_like(r)) for r in ref]
        for t, (r, gr) in enumerate(zip(ref, grads)):
            r.grad = None if t in dropped else gr * gscale  # (a power of two: exact)
        live = [r for r in ref if r.grad is not None]
        for r in live:
            if not torch.isfinite(r.grad).all():
                r.grad.zero_()
        norm64 = math.sqrt(sum(float(r.grad.double().pow(2).sum()) for r in live))
        eps_c = 0.0
        if clip is not None:
            tn = torch.nn.utils.clip_grad_norm_(live, clip)
            c_t = min(1.0, float(clip / (tn + 1e-6)))  # (as clip_grad_norm_ forms it: a Python float over a tensor)
            clip32 = float(torch.tensor(clip, dtype=torch.float32))  # (max_norm reaches both sides as an fp32 number)
            c_64 = min(1.0, float(torch.tensor(clip32 / (norm64 + 1e-6), dtype=torch.float32)))
            if c_t != 1.0 or c_64 != 1.0:  # (relative distance of the two coefficients; one rounding when they agree)
                eps_c = abs(c_t - c_64) / c_64 + 2.0 ** -24
        opt_ref.step()
        for t in range(T):
            steps_ref[t] += 0 if t in dropped else 1

        flat.zero_grad()
        for p, gr in zip(flat.params, grads):
            p._mvae_main_grad.copy_(gr.to(dev))
        snap = [x.clone() for x in (flat.data, flat.grad, opt.exp_avg, opt.exp_avg_sq)]
        opt.step(used=used.to(dev))
        torch.cuda.synchronize()
        data, grad, m, v = (x.cpu() for x in (flat.data, flat.grad, opt.exp_avg, opt.exp_avg_sq))
        snap = [x.cpu() for x in snap]

        assert opt.steps.cpu().tolist() == steps_ref, ("steps", it)
        tot = float(opt.last_total_norm)
        print(f"step {it}: total norm {tot!r} float64 {norm64!r} eps_c {eps_c:.3e}")
        assert abs(tot - norm64) <= 1e-6 * norm64, ("total norm", it, tot, norm64)
        for name, buf in (("p", data), ("g", grad), ("m", m), ("v", v)):
            pad = buf[~owned]
            assert not pad.any(), (name, "padding written", it)
        for t, (p, off) in enumerate(zip(flat.params, flat.offsets)):
            n = p.numel()
            sl = slice(off, off + n)
            what = f"step {it} tensor {t} ({tuple(shapes[t])})"
            if t in dropped:  # untouched, bitwise
                for name, buf, old in zip("pgmv", (data, grad, m, v), snap):
                    E.assert_exact(buf[sl].view(torch.int32), old[sl].view(torch.int32), "i", f"{what} {name} (unused)")
                continue
            r = ref[t]
            st = opt_ref.state[r]
            p0, m0, v0 = (_flat_of(x) for x in before[t])
            pr, gr_, mr, vr = _flat_of(r.detach()), _flat_of(r.grad), _flat_of(st["exp_avg"]), _flat_of(st["exp_avg_sq"])
            sp = torch.maximum(pr.abs(), p0.abs())
            sm = torch.maximum(torch.maximum(mr.abs(), m0.abs()), gr_.abs() + wd * p0.abs())
            sv = torch.maximum(vr, v0)
            # Error recursion of one step, from the bounds carried from the step before (carry[t] = bounds of p, m, v):
            # dg: the gradient entering the moments -- the clip coefficient's distance, and for L2 decay the rounding
            # of g + wd * p (contracted here, not in torch) and wd times the parameter's own bound;
            # m' = b1 m + (1 - b1) g and v' = b2 v + (1 - b2) g^2 carry b1 / b2 of their old bounds, take
            # (1 - b1) dg / (1 - b2) (2 |g| dg + dg^2), and round (K_STEP ulp of the larger operand).
            eg = eps_c + 2.0 ** -23 if eps_c else 0.0
            cp, cm, cv = carry.get(t, (0.0, 0.0, 0.0))
            gl2 = gr_.double() if decoupled else gr_.double() + wd * p0.double()
            dg = gr_.double().abs() * eg
            if not decoupled:
                dg = dg + E.ulp32(torch.maximum(gr_.abs(), wd * p0.abs())) + wd * cp
            bm = betas[0] * cm + (1 - betas[0]) * dg + K_STEP * E.ulp32(sm)
            bv = betas[1] * cv + (1 - betas[1]) * (2 * gl2.abs() * dg + dg * dg) + K_STEP * E.ulp32(sv)
            print(f"  {what}: ulps p {_ulps(data[sl], pr, sp):.2f} m {_ulps(m[sl], mr, sm):.2f} "
                  f"v {_ulps(v[sl], vr, sv):.2f} g {_ulps(grad[sl], gr_, gr_):.2f} (eps_c {eps_c:.2e})")
            if eps_c == 0.0:
                E.assert_exact(grad[sl], gr_, "i", f"{what} written-back gradient")
            else:
                E.assert_within(grad[sl], gr_, gr_.double().abs() * eg, "i", f"{what} written-back gradient")
            if it == 1 and t in (4, 7):
                assert not grad[sl].any(), (what, "non-finite gradient not zeroed")
            # p = p0' + (-step_size) * (m / denom): the final addition rounds in ulp(p); the update u itself carries the
            # absolute error of m through step_size / denom, the relative error of denom (exp_avg_sq's, halved by the
            # square root) and four more roundings (the division by bias_correction2_sqrt, + eps, m / denom, the product)
            k_step = steps_ref[t]
            ss = lr / (1 - betas[0] ** k_step)
            denom = vr.double().sqrt() / math.sqrt(1 - betas[1] ** k_step) + 1e-8
            u = ss * mr.double().abs() / denom
            # (relative error of sqrt(v) for an absolute error bv of v, without linearizing: next to a cancellation
            # in g + wd * p, bv is not small against v; 1 / (1 - rd) turns it into the quotient's)
            r_v = (bv / vr.double().clamp_min(1e-300)).clamp_max(1e30)
            rd = torch.maximum((1 + r_v).sqrt() - 1, 1 - (1 - r_v).clamp_min(0).sqrt())
            # (every element must stay checked: no reference exp_avg_sq may be so ill-conditioned that the bound on
            # the quotient is void)
            assert float(rd.max()) < 0.5, (what, "exp_avg_sq bound reaches half of exp_avg_sq", float(rd.max()))
            rq = rd / (1 - rd)
            bp = cp + K_STEP * E.ulp32(sp) + ss * bm / denom * (1 + rq) + u * (rq + 4 * 2.0 ** -23)
            E.assert_within(data[sl], pr, bp, "i", f"{what} p")
            E.assert_within(m[sl], mr, bm, "i", f"{what} exp_avg")
            E.assert_within(v[sl], vr, bv, "i", f"{what} exp_avg_sq")
            carry[t] = (bp, bm, bv)
