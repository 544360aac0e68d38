"""The optimiser the reference builds (runner_base.py:104-137: torch.optim.AdamW, two groups, eps 1e-8) run in float64, next to
elementwise error budgets for the fused fp32 AdamW of csrc/optim.hip.  Shared by tests/test_kernels_gpu.py, test_model_gpu.py and
test_dp_gpu.py.

Budgets.  u = 2^-24 is the fp32 unit roundoff (round to nearest; a cast of a double to float, a product, a quotient, a sqrtf and
an add each err by at most u relative; optim.hip is built with -ffp-contract=fast, which only removes roundings).  Alongside the
reference, per element and per step the element's module takes part in:

  m_abs = b1 * m_abs + (1 - b1) * |g|                       (m's absolute-value recurrence: m can cancel, its error cannot)
  e_m   = b1 * e_m + C_M * u * m_abs                         |m - m_ref| <= e_m
      C_M = 4: the roundings of beta1, (1-beta1), (1-beta1)*g and the final add, each at most u times a term <= m_abs.
  r_v   = r_v + C_V * u                                      |v - v_ref| <= r_v * v_ref   (every term is positive: no cancellation)
      C_V = 4: beta2 and beta2*v carry 2u on the old part; (1-beta2), (1-beta2)*g and *g 3u on the new one; the final add u.
  A     = lr / bc1 * m_abs / (sqrt(v_ref) / sqrt(bc2) + eps)        (the step's |Adam term| with m_abs in place of m)
  e_p   = e_p * (1 - lr*wd) + C_P * ulp(max(|p_old|, |p_new|)) + (e_m / m_abs + r_v / 2 + C_A * u) * A
      C_P = 2: the decay factor 1 - lr*wd (0.5 ulp of p), p * factor (0.5 ulp) and the final fused subtract (0.5 ulp), rounded up.
      C_A = 10: the casts of lr, bc1, sqrt(bc2) and eps, lr / bc1, sqrtf, the division by sqrt(bc2), the add of eps and m / denom
      (9 roundings, rounded up); m's error enters through e_m / m_abs, v's through half its relative error (the square root).

An element of a module that never took part, or a step that skipped it, keeps a zero budget there: p, m and v must hold their bits."""
import math

import torch

U = 2.0 ** -24
BETA1, EPS = 0.9, 1e-8
C_M, C_V, C_P, C_A = 4, 4, 2, 10


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """ulp of |x| as an fp32 number, elementwise, in float64."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).double()


class AdamWRef:
    """float64 torch.optim.AdamW (foreach=False, fused=False) over `pieces` (fp32 tensors: the initial values), piece i in the
    weight-decay group `wds[i]` (0.05 or 0), plus the budgets of the module docstring.  step(grads, lr): grads[i] None = the
    piece's module was unused this step (torch skips a parameter whose .grad is None: no decay, no moment update, no step)."""

    def __init__(self, pieces, wds, beta2: float = 0.999):
        self.beta2 = beta2
        self.params = [torch.nn.Parameter(p.detach().double().clone()) for p in pieces]
        self.wds = [float(w) for w in wds]
        groups = {}
        for prm, wd in zip(self.params, self.wds):
            groups.setdefault(wd, []).append(prm)
        self.opt = torch.optim.AdamW([{"params": ps, "weight_decay": wd} for wd, ps in groups.items()], lr=1e-3,
                                     betas=(BETA1, beta2), eps=EPS, foreach=False, fused=False)
        self.m_abs = [torch.zeros_like(p) for p in self.params]
        self.e_m = [torch.zeros_like(p) for p in self.params]
        self.e_p = [torch.zeros_like(p) for p in self.params]
        self.r_v = [0.0] * len(self.params)

    def seed_state(self, i: int, step: int, m, v) -> None:
        """Piece i starts as a parameter with `step` updates behind it and moments m, v (exact: zero budgets)."""
        prm = self.params[i]
        self.opt.state[prm] = {"step": torch.tensor(float(step)), "exp_avg": m.detach().double().clone().reshape(prm.shape),
                               "exp_avg_sq": v.detach().double().clone().reshape(prm.shape)}
        self.m_abs[i] = self.opt.state[prm]["exp_avg"].abs()

    def step(self, grads, lr: float) -> None:
        for grp in self.opt.param_groups:
            grp["lr"] = lr
        old = []
        for prm, g in zip(self.params, grads):
            prm.grad = None if g is None else g.detach().double().clone()
            old.append(None if g is None else prm.detach().abs().clone())
        self.opt.step()
        for i, prm in enumerate(self.params):
            if prm.grad is None:
                continue
            st = self.opt.state[prm]
            t = int(st["step"])
            ma = self.m_abs[i].mul_(BETA1).add_(prm.grad.abs(), alpha=1 - BETA1)
            em = self.e_m[i].mul_(BETA1).add_(ma, alpha=C_M * U)
            self.r_v[i] += C_V * U
            bc1, bc2s = 1 - BETA1 ** t, math.sqrt(1 - self.beta2 ** t)
            a = (lr / bc1) * ma / (st["exp_avg_sq"].sqrt() / bc2s + EPS)
            rel = torch.where(ma > 0, em / ma.clamp_min(1e-300), torch.zeros_like(ma)) + self.r_v[i] / 2 + C_A * U
            self.e_p[i].mul_(1 - lr * self.wds[i]).add_(C_P * ulp32(torch.maximum(old[i], prm.detach().abs()))).add_(rel * a)
            prm.grad = None

    def steps(self, i: int) -> int:
        st = self.opt.state.get(self.params[i], {})
        return int(st["step"]) if "step" in st else 0

    def check(self, i: int, p, m, v, what: str = "") -> None:
        """Piece i of the HIP state (fp32 p, m, v) against the reference, within the budgets."""
        prm = self.params[i]
        st = self.opt.state.get(prm, {})
        m_ref = st.get("exp_avg", torch.zeros_like(prm))
        v_ref = st.get("exp_avg_sq", torch.zeros_like(prm))
        for name, got, ref, bound in (("p", p, prm.detach(), self.e_p[i]), ("m", m, m_ref, self.e_m[i]),
                                      ("v", v, v_ref, self.r_v[i] * v_ref)):
            got = got.to(ref.device).double().reshape(ref.shape)
            err = (got - ref).abs()
            bad = ~(err <= bound)                     # a NaN or an inf is over any budget
            if bool(bad.any()):
                j = int(torch.argmax(torch.nan_to_num(err - bound, nan=math.inf).flatten()))
                raise AssertionError(f"{what} piece {i} {name}: {int(bad.sum())} elements over budget; worst at {j}: "
                                     f"got {float(got.flatten()[j])!r} ref {float(ref.flatten()[j])!r} "
                                     f"err {float(err.flatten()[j]):.3e} budget {float(bound.flatten()[j]):.3e}")
