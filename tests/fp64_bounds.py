"""Poisoned buffers and element-wise fp64 error bounds for the GEMM and attention kernels (shared by the CPU mutation tests and
the GPU edge tests).

Poison: a fixed NaN bit pattern (bf16 0x7FA5, f32 0x7FC0DEAD, int32 0xDEADBEEF).  A kernel that skips an element it owns leaves
the pattern there (NaN: never within a bound); a kernel that writes outside what it owns destroys it (`untouched` is False).

Bounds.  u16 = 2^-8 is bf16's unit roundoff (8 significant bits: round to nearest is within half an ulp, 2^-8 |x| at the
bottom of a binade), u32 = 2^-24 fp32's.  Every bound is a sum of (rounding points) x (the magnitude product the rounded value
is bounded by), never |ref| alone, so a row or head whose values are small next to the tensor's maximum gets a bound of its own
size:

GEMM, |got - ref| <= e with, for P = A B^T and |P| := |A| |B|^T,
    e_acc = alpha * g_acc(K, s) * |P|,  g_acc = (K/16 + s + 2) * u32
        fp32 accumulation of exact bf16 x bf16 products (16 x 8 significant bits fit fp32's 24): every MFMA adds at most 32
        products to the accumulator with one rounding of a partial sum bounded by |P| -- K/16 counts two per instruction, a
        margin of 2 over K/32 -- and the split reduce adds s - 1 slab roundings; + 2 for alpha and the slab read-out.
    + alpha * u16 * |P| when the split partials are bf16 slabs (one rounding per slab, each bounded by its part of |P|),
    + u32-sized roundings of bias / residual additions (2 u32 (|v| + |bias|)),
    gelu: the pre-activation bound times max|gelu'| = 1.13 plus the erf evaluation's error (the
        Abramowitz-Stegun erfc form, |err| <= 1.5e-7: 2e-7 |v| + 4 u32 |gelu(v)|),
    bf16 output: e' = e + u16 (|ref| + e).
Attention (the kernels round rotated q / k to bf16 once, P = exp(s - m) to bf16 before P V and dS to bf16 before dS K / dS^T Q):
    scores: ds_ij = scale g_acc(D) (|q||k|^T)_ij + 2 u32 |s_ij| + the rotation's rounding ambiguity, per element: an fp32
         rotation whose value lies within its own arithmetic error of a bf16 rounding midpoint may round either way, so such an
         element carries one bf16 ulp of uncertainty (rope_bf16: dq_e, dk_e; every other element is exact), giving
         scale (dq_e |k|^T + |q| dk_e^T + dq_e dk_e^T)_ij;
    o:   c_o,i (P|V|)_i with c_o,i = 2 u16 (P and the output rounded) + g_acc(Sk) + 2 max_j ds_ij;
    lse: max_j ds_ij + g_acc(Sk) + 4 u32 (|lse| + 1);
    backward, as a function of its inputs (q, k, v, the o and lse it is handed, dO): P = exp(s - lse) with relative error
         rho_ij = ds_ij + 2 u32 |s_ij - lse_i| + 4 u32; T = dP - delta, dP = dO v^T (error g_acc(D) |dO||v|^T), delta = rowsum(o dO)
         (error g_acc(D) rowsum(|o||dO|)); dS = P T with error e_dS = rho P |T| + P (e_dP + e_delta), then rounded to bf16
         (+ u16 (|dS| + e_dS));
         dq = scale dS k:   scale (e_dS |k| + g_acc(Sk) |dS||k| + |dS| dk_e),  dk likewise with q;
         dv = bf16(P)^T dO: ((u16 + rho) P)^T |dO| + g_acc(Sq) P^T |dO|;  each + u16 (|ref| + e) for the bf16 output.
         The dS error is bounded by P |dP - delta| -- the size of dS itself -- not by P |dO||v|^T: an error in one key tile
         or one row is then out of bound (tests/test_fp64_bounds_cpu.py shows it on an emulation of the kernels).
One-query decode attention (attn_decode_kernel, attn_decode_draft_kernel, one_row_attention; the split pair with `chunk`):
    decode_attn_ref_bound.  These kernels keep the probabilities in fp32 -- there is no u16 term on P|V|; the only bf16
    rounding is the output's.  With len = min(kv_len, T_cap) keys, P_j the fp64 probabilities and PV = sum_j P_j |v_j|:
    scores: qf = bf16(q) * scale is rounded once, a lane makes 8 serial multiply-adds (a product and a sum each, or one fused
        operation: 9 roundings with qf's at most), a 4-step butterfly over the key's 16 lanes follows:
        ds_j = G_SCORE u32 scale (|q||k_j|), G_SCORE = 1 + 1 + 8 + 4 = 14, + scale (dq_e |k_j| + |q| dk_e,j + dq_e dk_e,j) where
        the caller cannot read the rotated value back (q_err / k_err of rope_bf16, as in attn_ref_bound).
    weights: the kernel's weight of key j is w_j = __expf(fl(s'_j - mx')) with s' the computed scores and mx' their maximum.  A
        common factor of all w_j cancels between the numerator and the normaliser, so only the error relative to
        exp(s_j - mx') counts: 1 + rho_j = exp(x_j) (1 + eta_j) with x_j = ds_j + u32 |a_j| (the score's error and the rounded
        difference, both in the exponent) and |eta_j| <= (4 + 2 |a_j|) u32 (the __expf allowance above), |a_j| = max_i s_i - s_j
        + ds_j + max_i ds_i.  A weight below fp32's normal range may be flushed to zero: + 2^-126 absolute on every w_j (the
        largest is 1), 2 F32_TINY on P_j.  The same w_j enter the numerator and the normaliser, and for weights
        P_j (1 + rho_j) the normalised sum moves by exactly sum_j P_j rho_j (v_j - o) / (1 + sum_j P_j rho_j), so
        e_w = sum_j (P_j rho_j + 2 F32_TINY) |v_jd - o_d| / (1 - sum_j P_j rho_j): every key's error enters weighted by its own
        P_j, never as max_j rho_j -- a spike row whose other keys are far away keeps a bound of its own size.
    normaliser: a lane adds its ceil(len / 64) positive terms serially, then the 6-step butterfly: g_norm = (ceil(len / 64) + 6)
        u32, relative; inv = 1 / sum: C_FN u32; the product by inv: u32.
    PV: a wave adds its ceil(len / 16) keys serially (the product and the sum: ceil(len / 16) + 1), the 16 wave partials are added
        in order (16): g_pv = (ceil(len / 16) + 17) u32 on PV.
    o:  e = e_w + g_pv PV + (g_norm + (C_FN + 1) u32) (|o| + e_w), then the one bf16 rounding, e + u16 (|o| + e).
    lse = mx' + __logf(sum') = lse + log(1 + sum_j P_j (rho_j + phi_j)) before the function's own error:
        sum_j P_j rho_j + g_norm + C_FN u32 (|log sum| + 1) + u32 (|lse| + |max_j s_j|) -- at most max_j ds_j + the normaliser's
        relative error + the function's (the + 1: a relative error of sum' is an absolute one of its logarithm).
    len = 0: o is exactly 0 and lse exactly -inf (bound 0).
    split form (chunk = 128 / 256 / 512; attn_decode_split_kernel + attn_decode_combine_kernel): a chunk of n_c keys is the
        one-row kernel with 4 waves -- |a_j| counts from the chunk's own maximum, g_norm,c = ceil(n_c / 64) + 6, a wave adds
        ceil(n_c / 4) keys, the four partials are added in order: g_pv,c = ceil(n_c / 4) + 1 + 4.  The merge multiplies the record
        of chunk c by __expf(fl(m_c - M)): rho_c = (1 + 4 + 2 |m_c - M|) u32, a factor (1 + rho_c) on every weight of the chunk
        (rho_j + rho_c + rho_j rho_c takes rho_j's place; a flushed factor loses at most 2^-126 per key: 4 F32_TINY in all), and
        adds nc = ceil(len / chunk) products serially for L and for o: + nc + 1 on g_norm and on g_pv.

Row kernels (norm.hip, loss.hip, expert.hip l2norm): one 256-thread workgroup per row sums D terms in fp32 as per-thread serial
sums of float4 chunks (4 ceil(D/1024) terms a thread), a 64-lane butterfly (6 additions), then the wave values in order:
    g_sum(n_thread, n_waves) = (n_thread + 6 + n_waves + 4) * u32 on sum |terms|   (+ 4: the terms' own products / differences),
    g_row(D) = g_sum(4 ceil(D/1024), 4).
Math functions are not correctly rounded.  No HIP math accuracy table is installed next to the compiler this suite was written
against, so these are stated assumptions, not documented figures: expf, logf, rsqrtf, sqrtf and a division are each allowed
C_FN = 4 ulp (c_fn * u32 relative); the fast __expf(a) (an exp2 of a rounded a log2 e) is allowed (4 + 2 |a|) u32.
    rmsnorm: v = mean(x^2) + eps has relative error rho = g_row + 2 u32 (all terms positive), r = rsqrt(v) then
        rel_r = rho/2 (1 + 2 rho) + (C_FN + 1) u32; y = w x r: |y| (rel_r + 3 u32).  Backward dx = r w g - x cc + dres with
        cc = r^3 sum(x w g) / D: e_cc = r^3/D (g_row + 2 u32) sum|x w g| + (3 rel_r + 4 u32) |cc| -- the sum of magnitudes, so a row
        whose gradient cancels keeps a bound of its own size -- and e = (rel_r + 4 u32) |r w g| + |x| (e_cc + 2 u32 |cc|) + 2 u32 |dx|.
    layernorm: e_mean = g_row mean|x| + u32 |mean|; sum (x - m')^2 = sum (x - m)^2 + D (m - m')^2 exactly, so the mean's error
        enters the variance squared: e_var = e_mean^2 + (g_row + 6 u32) var, rho = e_var / (var + eps) (a row with rho > 1/2 must
        be constant: its reference deviation is exactly 0 and r' <= rsqrt(eps) still bounds the output), rel_r as above.
        y = d r w + b, d = x - m: |r w| e_mean + |d r w| (rel_r + 4 u32) + 2 u32 |y|.  Backward dx = r (gw - sg - xh sgx) + dres:
        e_xh = r e_mean + |xh| (rel_r + 2 u32), e_sg = (g_row + 2 u32) mean|gw|, e_sgx = (g_row + 4 u32) mean|gw xh| + mean(|gw| e_xh),
        e = r (e_sg + |sgx| e_xh + |xh| e_sgx + 4 u32 (|gw| + |sg| + |xh sgx|)) + |dx - dres| (rel_r + u32) + 2 u32 (|dx| + |dres|).
    layernorm_param_grads: dgamma = sum_m g xhat, dbeta = sum_m g: sum_m |g| e_xh + (16 + ceil(M/16) + 3) u32 sum_m |g xhat|
        (a column is summed serially over a block's 16 rows, then over the blocks), dbeta without the e_xh term.
    lowrank: see lowrank_ref_bound (block-sum dot products, R serial FMAs, chunked column sums over the rows).
    l2norm_rows: y = x / max(sqrt(sum x^2), eps): |y| (g_row / 2 + (2 C_FN + 2) u32).
    clamp_ce: p_j = exp(x_j - m) / se.  The difference x_j - m is rounded (u32 |x_j - m| absolute, so relative in the exponential),
        rel_se = g_sum + u32 sum_j p_j (C_FN + 1 + |x_j - m|), rho_j = rel_se + (C_FN + 4 + |x_j - m|) u32;
        dlogits_j = gs (p_j - [j = t]): gs (rho_j p_j + u32 |p_j - [j = t]|) + u32 |ref|, then the bf16 rounding; row_loss =
        -log(clamp(p_t)): rho_t + (C_FN + 1) u32 |loss|.  The clamp is a decision: a row whose p_t lies within rho_t p_t + 4 u32 of
        a threshold (fp32 1e-7, or fp32 1 - 1e-7 with 2 u32 more) may take either branch (clamp_ce_check accepts both for that
        row) -- but a row whose label holds the maximum while all other exponentials sum to < u32 / 2 has p_t = 1 in fp32 in
        any summation order (1 + d rounds to 1) and is saturated for certain.  Rows without
        a label (t < 0 or t >= V) and the pad columns V..ldd are exactly zero.
    sum_f32: g_sum(ceil(n/256), 4) sum|x| + u32 |ref|; argmax margin: u32 |margin| (ids exact, first index on ties);
        p_max = 1 / sum __expf(a_j): g_sum + u32 sum_j p_j (4 + 2 |a_j|) + (C_FN + 1) u32, relative.
Elementwise (elementwise.hip; bf16 in, fp32 arithmetic, one bf16 rounding out):
    silu_mul: s = 1 / (1 + __expf(-g)) has rel_s = (4 + 2 |g|) u32 (1 - s) + 3 u32; h = g s u: |h| (rel_s + 3 u32).  Backward
        du = d g s likewise; dg = d u f, f = s + g s (1 - s): e_f = s rel_s + |g| s (1 - s) (rel_s + 2 u32) + |g| s (s rel_s + u32)
        + u32 (|f| + |g s (1 - s)|), e = |d u| e_f + 3 u32 |dg|.  (+ 2^-126 absolute: fp32 underflow of the far negative tail.)
    gelu: the erfc form's allowance of the GEMM epilogue (4 u32 |gelu| + 2e-7 |x|); backward dy (cdf + x pdf):
        |dy| (2e-7 + |x| pdf (4 + x^2) u32 + 4 u32 |gelu'|) + u32 |ref|.
    rope_: rope_bf16 (sign = -1 for the backward): a bf16-valued reference plus a one-ulp ambiguity mask.
    dropout_bf16 / dropout_add_: the keep mask regenerated by the library, then one fp32 product and the output rounding
        (u32 |ref| then bf16) or the sum's (u32 |dy keep| + u32 |ref|).
    Data movement (copies, gathers, scatters, casts, transposes, patchify, decode records): no bound, torch.equal; accumulate
        forms u32 (|a| + |b|).
Conv stack (conv.hip).  Data movement, compared by value with torch.equal (bit equality but for the sign of a zero):
    im2col: an index gather in (ky, kx, c) order (im2col_ref; not F.unfold, whose columns are channel-major): column K is exactly
        1.0 with the bias column, every other column >= K exactly 0, every out-of-image tap exactly 0.
    conv_pack: bf16(W) rounded to nearest even, the bf16 bias at column K (if any), zeros after it.  conv_unpack_grad: a copy of
        the columns < K and of column K.
    relu_pool_fwd: bf16(max(0, max of the four)).  fmaxf(0.f, -0.f) may return either zero, so a window whose maximum is a
        zero is compared by value (torch.equal does: -0 == 0).
    relu_pool_bwd: bf16(dp) at the first maximum of the window in the order (0,0), (0,1), (1,0), (1,1) iff that maximum is > 0
        (an argmax over a [.., 4] view, first index on ties; -0.0 == 0.0 is a tie and neither is > 0); zero at the other three
        cells and in the pad columns.
    col2im: the fp64 fold of the bf16 dcol.  The kernel adds up to kh kw exact bf16 values serially in fp32:
        (kh kw) u32 sum_taps |dcol| per element (an element no tap reaches, or whose taps are all zero, is exactly 0).
Map heads (expert.hip):
    pair_logits: scale <p, t_j> / ||p||.  A lane sums 4 ceil(C/256) products serially, then the 64-lane butterfly (no wave
        values to add: g_sum(4 ceil(C/256), 0)); the same sum gives ||p||^2 (all terms positive: relative, halved by the square
        root), then sqrtf, one division and the product:
        (scale / ||p||) g_sum sum_i |p_i t_i| + |ref| (g_sum / 2 + (2 C_FN + 2) u32).
    bilinear_ac: the reference's source position is the exact rational oy (h-1) / (H-1) in fp64; a kernel's is oy fl(step) in
        fp32 (zs_accumulate; bilinear_ac divides the exact integers once), a relative error of at most 2 u32 of a value <= h - 1.  The interpolant is continuous and piecewise linear, so a
        position error d moves it by at most d times the slope |in[y1] - in[y0]| (interpolated along the other axis) of the cell
        the position lies in or of the cell next to it -- the largest over the 3 x 3 neighbourhood of cells is taken, so an
        (int)fy that lands in the neighbouring cell needs no exemption.  The lerp itself: 6 u32 on the sum of the four weighted
        magnitudes (1 - w, the product, the inner sum, 1 - v, the product, the outer sum); one_minus: + u32 |1 - v|.
    zs_accumulate, map: d = l1 - l0 is rounded (u32 |d|, interpolated with the same weights: one more u32 on the weighted
        magnitudes), then the position and lerp errors above give e_d; through the sigmoid (slope s (1 - s) e^e_d <= 1/4) plus
        the sigmoid's own relative error (_sigmoid_rel: the __expf allowance and three roundings); then acc + w s:
        u32 (|acc| + |w s|).  mask: the same with e_d = u32 |d| (no interpolation).
    rowmax_skip: the maximum over the kept columns is exact; acc + w m has two roundings: 2 u32 (|acc| + |w m|).  A row whose
        kept maximum is -inf gives exactly -inf.
    Pool routing in a chain (conv GEMM -> pool): a window whose fp64 runner-up lies within the GEMM bounds of the maximum, or
        whose maximum lies within its bound of 0, may route either way (pool_decisions); the chain test gives such windows no
        gradient and asserts they are at most 1 % of all windows.
LoRA (lora.hip).  The dropout mask is stated independently of the library: keep_mask_ref restates common.h's dropout_hash /
    dropout_hash2 / dropout_keep in integer arithmetic; v_proj's mask is the second draw of q_proj's hash (seed bit 63).  The
    kernels multiply by bf16(A) (the forward's MFMA operand), so every reference does.  ik = 1 / (1 - p) is an fp32 quotient,
    allowed C_FN ulp like every division here.
    lora_down: group g < G, column j holds s ik sum_{d in [g D/G, (g+1) D/G)} keep(m,d) x[m,d] bf16(A)[j,d] (q mask for j < R2/2,
        v mask otherwise; dropped elements are zeroed, exact).  A workgroup's 8 waves split the group's k-steps, each an MFMA
        chain of 32-product blocks; the 8 partial sums are added like split-K slabs:
        s ik g_acc(D/G, 8) sum |keep x bf16(A)| + (C_FN + 3) u32 |ref| (ik, the scale, the product), then the bf16 rounding.  The
        sum across the groups (the qkv GEMM forms it) carries the sum of the groups' bounds.
    lora_dx: base + s (kq sum_{j<r} g_j a_j + kv sum_{j>=r} g_j a_j), a = bf16(A): each half is r serial FMAs, then the two mask
        products folded into one FMA and the outer FMA: (r + 3) u32 s (kq sum |g_j a_j| + kv sum |g_j a_j|), + (C_FN + 1) u32 on
        the same term when p > 0 (ik), + u32 |ref|.  base and g enter as given (the slab sums that form them are exact in the
        tests: integer products).
    lora_wgrad, as a function of what it reads (bf16 x, the fp32 border gradient g, the bf16 border summed over its 64 / R2
        groups, bf16 dq / dv): dA[j,d] = sum_m s g[m,j] keep(m,d) x[m,d], dB_q[d,j] = sum_m dq[m,d] st[m,j], dB_v likewise.
        st = the groups added in order: 3 u32 sum |groups|, carried through |dq| / |dv|.  Thread-per-column kernel: 64 row chunks,
        a chunk's ceil(M/64) rows added serially, the chunks added in order, + 4 for the scalar, the mask product and the FMA:
        (ceil(M/64) + 64 + 4) u32 on sum_m of the magnitudes.  MFMA kernel (r = 8, D % 128 == 0): the per-row scalars are a bf16
        head plus a bf16 remainder (relative error u16^2), two MFMAs per 32-row step at two roundings each as g_acc counts them,
        16 chunks, ik applied to the finished sum: (u16^2 + (4 ceil(ceil(M/16)/32) + 16 + C_FN + 4) u32) on the same magnitudes.
        A gradient that cancels over the rows keeps the bound of its terms.
    lora_refresh_border(s): data movement, torch.equal against bf16(B) in every group of W_ext and W_ext^T; every other cell
        untouched (lora_refresh_check).
    rmsnorm backward behind lora_dx: rmsnorm_ref_bound(dy_err=...) carries the bound of d(xn) through the norm (dx is linear in
        dy): r |w| e + |x| r^3 / D sum |x w| e.
Q-Former training (the DROP instances of attention.hip, qf_dropout.hip, wgrad.hip's TN GEMM).  Every mask is keep_mask_ref; its
    factor Z is 0 or the fp32 quotient 1 / (1 - p) (a correctly rounded division: the same value on both sides).
    attention dropout, attn_ref_bound(keep=Z [B, H, Sq, Sk]): the forward sums the undropped exponentials e (lse is unchanged),
        forms e z in fp32 (one more rounding: c_o gains u32), rounds to bf16 and multiplies by v: o = (P o Z) v with
        c_o (P o Z)|v|.  Backward, from the dropped o it is handed: delta = rowsum(o dO) = sum_j P_ij Z_ij (dO v^T)_ij, so
        dS = P (Z o dP - delta) with dP = dO v^T; the kernels form dP z in fp32: e_dP = Z o ((g_acc(D) + u32) |dO||v|^T), a
        dout_err term likewise times Z; e_dS, dq and dk follow unchanged.  dv = bf16(P_b o Z)^T dO: the error terms carry P_b o Z
        and u32 (the product e z) beside u16.  An element whose mask is flipped moves dS by P ik |dP| there: out of bound where
        P is not small (tests/test_fp64_bounds_cpu.py).
    layernorm dropout: x = z keep_in + res: 2 u32 (|z keep_in| + |x|) (a product and a sum, or one fused operation); the
        statistics come from the fp32 x the kernel wrote, so the LayerNorm reference takes that x_out as its input;
        y = LN(x_out) keep_out: keep_out y_bound + u32 |y|, then the bf16 rounding.  The sums are per-thread serial sums of
        ceil(D / 256) scalar terms -- never more than g_row's 4 ceil(D / 1024).  Backward: g = dy keep_out is one product,
        dy_err = u32 |g| through layernorm_ref_bound(dy_err=...): dx is linear in dy, a dy moved by e moves it by at most
        r (|w| e + mean(|w| e) + |xh| mean(|w| e |xh|)); dz = bf16(dx keep_in): keep_in e + u32 |dz|, then the rounding.
    tn_wgrad: dW = dy^T x over the rows: a split adds one MFMA (32 exact products, one rounding; g_acc counts two) per 32-row
        step and the splits are added in split order: g_acc(M, splits) |dy|^T |x| (+ u32 |dW| onto an earlier value).  db: a
        staging thread adds its column over the steps of its split, the 32 staging rows are added in order, then the splits:
        (ceil(rows_per / 32) + 32 + splits + 1) u32 sum_m |dy| (+ u32 |db| onto an earlier value).
"""
from __future__ import annotations

import contextlib

import torch

U16 = 2.0 ** -8
U32 = 2.0 ** -24

_INT_VIEW = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32}
POISON = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FC0DEAD, torch.int32: -0x21524111}     # -0x21524111 == 0xDEADBEEF as int32


def poison_(t: torch.Tensor) -> torch.Tensor:
    """Fill t (any strides) with its dtype's poison bits; returns t."""
    t.view(_INT_VIEW[t.dtype]).fill_(POISON[t.dtype])
    return t


def poisoned(shape, dtype, device) -> torch.Tensor:
    return poison_(torch.empty(shape, dtype=dtype, device=device))


def untouched(t: torch.Tensor) -> torch.Tensor:
    """Boolean mask: True where t still holds the exact poison bits."""
    return t.view(_INT_VIEW[t.dtype]) == POISON[t.dtype]


def assert_untouched(t: torch.Tensor, what: str = ""):
    ok = untouched(t)
    if not bool(ok.all()):
        idx = tuple(int(i) for i in (~ok).nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} element(s) outside the owned window were written, first at {idx} "
                             f"= {t[idx].item()!r}")


@contextlib.contextmanager
def poisoned_allocations(monkeypatch, device_type: str = "cuda"):
    """While active, torch.empty / torch.empty_like return poisoned tensors on `device_type` (bf16, f32, int32): the outputs and
    scratch a wrapper allocates start as NaN, not as whatever the caching allocator last held there.  Build references outside."""
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.device.type == device_type and t.dtype in POISON:
            poison_(t)
        return t

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", lambda *a, **k: fill(empty(*a, **k)))
        m.setattr(torch, "empty_like", lambda *a, **k: fill(empty_like(*a, **k)))
        yield


def assert_within(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """|got - ref| <= bound element by element (NaN fails).  Returns max err / bound; on failure names the worst element."""
    got64, ref64 = got.double(), ref.double()
    bound64 = torch.broadcast_to(bound.double(), ref64.shape)
    err = (got64 - ref64).abs()
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bound64.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        flat = int(ratio.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        nbad = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: {nbad} of {ratio.numel()} elements out of bound; worst at {idx}: got {got64[idx].item():.8g} "
                             f"ref {ref64[idx].item():.8g} err {err[idx].item():.3g} bound {bound64[idx].item():.3g} "
                             f"err/bound {ratio[idx].item():.3g}")
    return worst


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------- GEMM
def g_acc(K: int, splits: int = 1) -> float:
    return (K / 16 + splits + 2) * U32


def gemm_ref_bound(a, b, *, alpha=1.0, bias=None, residual=None, gelu=False, out_bf16=False, splits=1, bf16_slabs=False):
    """(ref, bound) in fp64 for out = [residual +] act(alpha * a @ b^T [+ bias]) from bf16 operands (see the module docstring)."""
    a64, b64 = a.double(), b.double()
    P = a64 @ b64.T
    Pabs = a64.abs() @ b64.abs().T
    K = a.shape[1]
    v = alpha * P
    e = abs(alpha) * (g_acc(K, splits) + (U16 if bf16_slabs else 0.0)) * Pabs + U32 * v.abs()
    if bias is not None:
        v = v + bias.double()
        e = e + 2 * U32 * (v.abs() + bias.double().abs())
    if gelu:
        pre = v
        v = torch.nn.functional.gelu(v)
        e = 1.13 * e + 4 * U32 * v.abs() + 2e-7 * pre.abs()
    if residual is not None:
        v = v + residual.double()
        e = e + 2 * U32 * v.abs()
    if out_bf16:
        e = e + U16 * (v.abs() + e)
    return v, e


# ---------------------------------------------------------------------------------------------------------------- attention
def rope64(x, pos, cos, sin, sign=1.0):
    """Rotate-half rotary (modeling_llama.py:109-123) in x's dtype: x [B, H, S, D], pos [B, S] long, tables [max_pos, D/2]."""
    D = x.shape[-1]
    c = torch.cat([cos[pos], cos[pos]], -1)[:, None].to(x.dtype)
    s = torch.cat([sin[pos], sin[pos]], -1)[:, None].to(x.dtype) * sign
    rot = torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    return x * c + rot * s


def rope_abs_map(bnd, pos, cos, sin):
    """Bound of R^T g given a bound of g (element-wise): |c| b_d + |s| b_partner."""
    D = bnd.shape[-1]
    c = torch.cat([cos[pos], cos[pos]], -1)[:, None].to(bnd.dtype).abs()
    s = torch.cat([sin[pos], sin[pos]], -1)[:, None].to(bnd.dtype).abs()
    partner = torch.cat([bnd[..., D // 2:], bnd[..., :D // 2]], -1)
    return c * bnd + s * partner


def rope_bf16(x, pos, cos, sin, sign=1.0):
    """(bf16-valued fp64 rotation of bf16 x, per-element uncertainty): a kernel rotates in fp32 and rounds once.  Where the fp64
    value lies within 8 u32 of the magnitudes (|x c| + |x' s|) of a rounding midpoint, the kernel's fp32 value may round to the
    other neighbour: that element carries one ulp; every other element rounds as the reference does -- except where x c and
    x' s cancel so far that the arithmetic error is no longer small against the result's own ulp (see below)."""
    x64 = x.double()
    c64, s64 = cos.double(), sin.double()
    r = rope64(x64, pos, c64, s64, sign)
    mag = rope_abs_map(x64.abs(), pos, c64, s64)
    rb = r.float().to(torch.bfloat16).double()
    lo = torch.ldexp(torch.ones_like(r), torch.frexp(r.abs().clamp_min(1e-30))[1] - 8)      # ulp of r's binade (8 bits)
    near_mid = torch.zeros_like(r, dtype=torch.bool)
    for ulp in (lo / 2, lo, 2 * lo):                                                      # a rounding across a binade edge too
        near_mid |= ((r - rb).abs() - ulp / 2).abs() <= 8 * U32 * mag
    ulp = 2 * lo
    unc = torch.where(near_mid, ulp, torch.zeros_like(r))
    # cancellation: where the fp32 arithmetic error itself reaches a quarter of the value's bf16 ulp the result can land several
    # ulps away -- such an element carries that error plus the rounding of wherever it lands
    arith = 8 * U32 * mag
    return rb, torch.where(arith >= lo / 4, arith * (1 + 2 * U16) + ulp, unc)


def attn_mask(B, Sq, Sk, causal, kv_len, device):
    """True where key j is visible to query i: [B, 1, Sq, Sk] (causal aligns the last query with the last key)."""
    i = torch.arange(Sq, device=device)[:, None] + (Sk - Sq)
    j = torch.arange(Sk, device=device)[None]
    m = torch.ones(B, 1, Sq, Sk, dtype=torch.bool, device=device)
    if causal:
        m = m & (j <= i)[None, None]
    if kv_len is not None:
        m = m & (j[None, None] < kv_len.to(device).long()[:, None, None, None])
    return m


def _out_round(ref, e):
    return e + U16 * (ref.abs() + e)


def attn_ref_bound(q, k, v, scale, mask, q_err=None, k_err=None, dout=None, dout_err=None, o_in=None, lse_in=None, keep=None):
    """fp64 attention of bf16-valued q, k, v [B, H, S, D] (q, k as the kernel multiplies them: rotated and rounded, with the
    per-element uncertainties q_err / k_err of rope_bf16) and the visibility mask [B, 1, Sq, Sk].  Returns a dict: o, lse and
    their bounds; with dout [B, H, Sq, D] also dq, dk, dv (w.r.t. the given q, k, v) and their bounds -- the backward of the
    o / lse it is handed (o_in, lse_in: what the kernel's backward reads; default the exact ones).  dout_err bounds an error
    dout itself carries (a product rounded to bf16).  *_bound_acc: the bounds before the output's bf16 rounding.
    keep: the attention-probability dropout factor Z [B, H, Sq, Sk] (0 or the fp32 quotient 1 / (1 - p)): o = (P o Z) v with
    the lse of the undropped P, and the backward of that (module docstring); o_in is then the dropped output."""
    q, k, v = q.double(), k.double(), v.double()
    Z = None if keep is None else keep.double()
    qe = torch.zeros_like(q) if q_err is None else q_err.double()
    ke = torch.zeros_like(k) if k_err is None else k_err.double()
    D, Sq, Sk = q.shape[-1], q.shape[-2], k.shape[-2]
    kT = k.transpose(-1, -2)
    s = (q @ kT) * scale
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    PZ = P if Z is None else P * Z
    o = PZ @ v
    Vabs = v.abs()
    PV = PZ @ Vabs
    ds = (g_acc(D) * (q.abs() @ k.abs().transpose(-1, -2)) + qe @ k.abs().transpose(-1, -2) + q.abs() @ ke.transpose(-1, -2)
          + qe @ ke.transpose(-1, -2)) * scale
    ds = (ds + 2 * U32 * s.abs().masked_fill(~mask, 0.0)).masked_fill(~mask, 0.0)
    ds_row = ds.amax(-1)                                                             # [B, H, Sq]
    c_o = 2 * U16 + g_acc(Sk) + 2 * ds_row
    if Z is not None:
        c_o = c_o + U32                                                              # the fp32 product e z
    out = dict(o=o, lse=lse, o_bound=c_o[..., None] * PV + U32 * U16 * PV,
               lse_bound=ds_row + g_acc(Sk) + 4 * U32 * (lse.abs() + 1))
    if dout is None:
        return out
    o_b = o if o_in is None else o_in.double()
    lse_b = lse if lse_in is None else lse_in.double()
    g = dout.double()
    gabs = g.abs()
    Pb = torch.exp(s - lse_b[..., None])                                            # masked: exp(-inf) = 0
    rho = (ds + 2 * U32 * (s - lse_b[..., None]).abs().masked_fill(~mask, 0.0) + 4 * U32).masked_fill(~mask, 0.0)
    dP = g @ v.transpose(-1, -2)
    if Z is not None:
        dP = Z * dP
    delta = (g * o_b).sum(-1, keepdim=True)
    T = dP - delta
    dS = Pb * T
    GV = gabs @ Vabs.transpose(-1, -2)
    e_dP = g_acc(D) * GV
    e_delta = g_acc(D) * (gabs * o_b.abs()).sum(-1, keepdim=True)
    if dout_err is not None:                                                         # dS is linear in dO
        e = dout_err.double()
        e_dP = e_dP + e @ Vabs.transpose(-1, -2)
        e_delta = e_delta + (e * o_b.abs()).sum(-1, keepdim=True)
    if Z is not None:                                                                # dP z: one more fp32 product
        e_dP = Z * (e_dP + U32 * GV)
    e_dS = rho * Pb * T.abs() + Pb * (e_dP + e_delta)
    e_dS = e_dS + U16 * (dS.abs() + e_dS)                                            # dS rounded to bf16
    dSa = dS.abs()
    dq = scale * dS @ k
    dk = scale * dS.transpose(-1, -2) @ q
    PbZ = Pb if Z is None else Pb * Z                                                # what the dV product multiplies, before its bf16 rounding
    dv = PbZ.transpose(-1, -2) @ g
    e_dq = scale * (e_dS @ k.abs() + g_acc(Sk) * (dSa @ k.abs()) + dSa @ ke)
    e_dk = scale * (e_dS.transpose(-1, -2) @ q.abs() + g_acc(Sq) * (dSa.transpose(-1, -2) @ q.abs()) + dSa.transpose(-1, -2) @ qe)
    if Z is None:
        e_dv = (((U16 + rho * (1 + U16)) * Pb).transpose(-1, -2) @ gabs + g_acc(Sq) * (Pb.transpose(-1, -2) @ gabs))
    else:                                                                            # + u32: the fp32 product e z
        e_dv = (((U16 + U32 + rho * (1 + U16)) * PbZ).transpose(-1, -2) @ gabs + g_acc(Sq) * (PbZ.transpose(-1, -2) @ gabs))
    if dout_err is not None:
        e_dv = e_dv + PbZ.transpose(-1, -2) @ dout_err.double()
    out.update(dq=dq, dk=dk, dv=dv, dq_bound_acc=e_dq, dk_bound_acc=e_dk, dv_bound_acc=e_dv,
               dq_bound=_out_round(dq, e_dq), dk_bound=_out_round(dk, e_dk), dv_bound=_out_round(dv, e_dv))
    return out


G_SCORE = 14               # roundings of a one-query decode score: qf, 8 products folded into 8 sums (+ 1), a 4-step butterfly
DECODE_WAVES = 16          # attn_one_query.h OQ_WAVES: waves that share the keys of a one-row workgroup
SPLIT_WAVES = 4            # attn_decode_split.hip: waves of a chunk workgroup


def decode_attn_ref_bound(q, k, v, scale, kv_len, q_err=None, k_err=None, chunk=None):
    """fp64 one-query attention with fp32 probabilities (module docstring, "One-query decode attention"): q [B, H, D] and
    k, v [B, H, T, D] bf16-valued (q, k as the kernel multiplies them: rotated and rounded; q_err [B, H, D] / k_err [B, H, T, D]
    rope_bf16's uncertainties where the caller cannot read the device's rotation back), scale the launcher's float argument,
    kv_len [B] ints (clamped to T here as the kernels clamp it; the keys at and past it are never read and may hold anything).
    chunk: the split kernels' chunk size (None: the one-row kernels).  Returns a dict: o [B, H, D], lse [B, H], o_bound (after the
    bf16 rounding), o_bound_acc (before it), lse_bound.  A row with no key: o = 0, lse = -inf, bounds 0."""
    q, k, v = q.double(), k.double(), v.double()
    B, H, T, D = k.shape
    dev = k.device
    lens = torch.as_tensor(kv_len, device=dev).long().clamp(0, T)
    mask = (torch.arange(T, device=dev)[None] < lens[:, None])[:, None]                  # [B, 1, T]
    live = (lens > 0)[:, None]                                                           # [B, 1]
    k = torch.where(mask[..., None], k, torch.zeros_like(k))                             # rows past kv_len: poison, never read
    v = torch.where(mask[..., None], v, torch.zeros_like(v))
    qe = torch.zeros_like(q) if q_err is None else q_err.double()
    ke = torch.zeros_like(k) if k_err is None else torch.where(mask[..., None], k_err.double(), torch.zeros_like(k))
    sc = f32_value(scale)
    s = torch.einsum("bhd,bhtd->bht", q, k) * sc
    qk_abs = torch.einsum("bhd,bhtd->bht", q.abs(), k.abs())
    ds = sc * (G_SCORE * U32 * qk_abs + torch.einsum("bhd,bhtd->bht", qe, k.abs()) + torch.einsum("bhd,bhtd->bht", q.abs(), ke)
               + torch.einsum("bhd,bhtd->bht", qe, ke))
    ds = ds.masked_fill(~mask, 0.0)
    ninf = float("-inf")
    sm = s.masked_fill(~mask, ninf)
    m = sm.amax(-1, keepdim=True)
    m = torch.where(live[..., None], m, torch.zeros_like(m))
    e = torch.exp(sm - m)                                                                # masked: 0
    S = e.sum(-1, keepdim=True).clamp_min(1e-300)
    P = e / S
    lse = torch.where(live, m[..., 0] + S[..., 0].log(), torch.full_like(S[..., 0], ninf))
    o = torch.einsum("bht,bhtd->bhd", P, v)
    n_max = int(lens.max()) if lens.numel() else 0
    if chunk is None:
        m_own, rho_c, tiny = m, 0.0, 2 * F32_TINY
        n_norm = -(-n_max // 64) + 6
        n_pv = -(-n_max // DECODE_WAVES) + 1 + DECODE_WAVES
    else:
        nch = -(-T // chunk)
        pad = nch * chunk - T
        m_c = torch.nn.functional.pad(sm, (0, pad), value=ninf).view(B, H, nch, chunk).amax(-1)          # [B, H, nch]
        used = m_c > ninf
        m_c = torch.where(used, m_c, m.expand_as(m_c))
        rho_c = ((5 + 2 * (m - m_c)) * U32).repeat_interleave(chunk, -1)[..., :T]
        m_own = m_c.repeat_interleave(chunk, -1)[..., :T]
        tiny = 4 * F32_TINY
        n_c, nc = min(chunk, n_max), -(-n_max // chunk)
        n_norm = -(-n_c // 64) + 6 + nc + 1
        n_pv = -(-n_c // SPLIT_WAVES) + 1 + SPLIT_WAVES + nc + 1
    a_abs = ((m_own - s).clamp_min(0.0) + ds + ds.amax(-1, keepdim=True)).masked_fill(~mask, 0.0)
    x = ds + U32 * a_abs
    rho = torch.expm1(x) + (4 + 2 * a_abs) * U32 * torch.exp(x)
    rho = (rho + rho_c + rho * rho_c).masked_fill(~mask, 0.0)
    w_err = (P * rho + tiny).masked_fill(~mask, 0.0)                                     # [B, H, T]
    r_sum = (P * rho).sum(-1)                                                            # [B, H]
    if not bool((r_sum < 0.5).all()):
        raise ValueError("decode_attn_ref_bound: the weights' relative error is not small (rope ambiguity on a whole row?)")
    dev_v = (v - o[:, :, None]).abs()
    e_w = torch.einsum("bht,bhtd->bhd", w_err, dev_v) / (1 - r_sum)[..., None]
    PV = torch.einsum("bht,bhtd->bhd", P, v.abs())
    e_o = e_w + n_pv * U32 * PV + (n_norm + C_FN + 1) * U32 * (o.abs() + e_w)
    logS = S[..., 0].log()
    e_lse = r_sum + n_norm * U32 + C_FN * U32 * (logS.abs() + 1) + U32 * (torch.where(live, lse, torch.zeros_like(lse)).abs() + m[..., 0].abs())
    e_lse = torch.where(live, e_lse, torch.zeros_like(e_lse))
    e_o = torch.where(live[..., None], e_o, torch.zeros_like(e_o))
    return dict(o=o, lse=lse, o_bound_acc=e_o, o_bound=_out_round(o, e_o), lse_bound=e_lse)


def decode_attn_inputs(B, H, D, T_cap, seed, ld_pad=8):
    """Seeded host inputs of a one-query decode case: qkv [B, 3W + ld_pad] bf16 ~ 0.7 N(0, 1) with a border, cache
    [B, T_cap, 2W] bf16 of the same law (the caller poisons rows past kv_len), rotary tables to T_cap + 8 positions."""
    W = H * D
    qkv = (rnd(B, 3 * W + ld_pad, seed=seed) * 0.7).to(torch.bfloat16)
    cache = (rnd(B, T_cap, 2 * W, seed=seed + 1) * 0.7).to(torch.bfloat16)
    cos, sin = rope_tables(D, max_pos=T_cap + 8)
    return qkv, cache, cos, sin


# The grids of tests/test_decode_attention_edges_gpu.py, here so that tests/test_fp64_bounds_cpu.py checks the emulations at the
# same lengths and the rope ambiguity of the same seeds.  One-row kernel: 16 waves (OQ_WAVES), 128 keys per score pass in two 64-key
# halves, a 64-lane stride in the softmax, a 16-key wave round-robin with an 8 x 16 = 128-key unrolled group (taken while
# j + 112 < len: first at len = 113) and a remainder of up to 7 keys a wave.
DECODE_T = 257
DECODE_LENS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 112, 113, 127, 128, 129, 143, 144, 145, 255, 256, 257)
DECODE_DS = (8, 16, 40, 64, 88, 96, 128)
DECODE_HS = (1, 3)
SPLIT_CHUNKS = (128, 256, 512)
SPLIT_DS = (8, 40, 128)
DRAFT_KS = (1, 3, 8)
DRAFT_DS = (16, 48, 128)


def decode_seed(D, H):
    return 7000 + 10 * D + H


def decode_launches():
    """[(T_cap, kv_len[3], pos[3])] of the one-row grid: DECODE_LENS three at a time at T_cap = 257 (the last group adds
    T_cap + 5, which the kernel clamps), then T_cap == kv_len for 1, 64 and 65 with T_cap + 5 and T_cap - 1 beside it.  pos[b] =
    min(kv_len, T_cap) - 1 (0 for a row without a key) is row b's rotary position, and its cache row in the rows form."""
    out = []
    lens = list(DECODE_LENS) + [DECODE_T + 5]
    for i in range(0, len(lens), 3):
        out.append((DECODE_T, lens[i:i + 3]))
    for T in (1, 64, 65):
        out.append((T, [T, T + 5, T - 1]))
    return [(T, ls, [max(min(n, T) - 1, 0) for n in ls]) for T, ls in out]


DECODE_EDGE_KINDS = ("q_zero", "spike_50", "scores_200", "v_alternating")
DECODE_EDGE_LENS = [129, 257, 17]
DECODE_EDGE_SPIKE_ROW = 7


def decode_edge_inputs(kind, B, H, D, T_cap, seed, pos, spike_row=DECODE_EDGE_SPIKE_ROW, spike=50.0):
    """decode_attn_inputs with one score / value edge: q = 0 (uniform weights); cache key `spike_row` = c q_rot with c chosen so
    that its score is `spike` (the others are ~0.5 N(0, 1)); q scaled by 400 (scores ~200 N(0, 1)); v = (-1)^j (1 + 0.01 N(0, 1))
    so that |o| << P|V|.  pos [B]: the rotary positions of q (the spike is a multiple of the rotated q)."""
    W = H * D
    qkv, cache, cos, sin = decode_attn_inputs(B, H, D, T_cap, seed)
    if kind == "q_zero":
        qkv[:, :W] = 0
    elif kind == "scores_200":
        qkv[:, :W] = (qkv[:, :W].float() * 400).to(torch.bfloat16)
    elif kind == "v_alternating":
        sign = torch.where(torch.arange(T_cap) % 2 == 0, 1.0, -1.0)[None, :, None]
        cache[..., W:] = (sign * (1 + 0.01 * cache[..., W:].float())).to(torch.bfloat16)
    elif kind == "spike_50":
        q = qkv[:, :W].float().view(B, 1, H, D).transpose(1, 2)
        qrot = rope64(q, torch.as_tensor(pos)[:, None], cos, sin).to(torch.bfloat16).float()[:, :, 0]           # [B, H, D]
        c = spike / (f32_value(D ** -0.5) * (qrot * qrot).sum(-1, keepdim=True))
        cache[:, spike_row, :W] = (c * qrot).reshape(B, W).to(torch.bfloat16)
    else:
        raise ValueError(kind)
    return qkv, cache, cos, sin


def decode_rope_pair(qkv, H, D, pos, cos, sin):
    """rope_bf16 of the q and k columns of qkv rows [R, >= 3W] at pos [R]: (qr, qe, kr, ke), each [R, H, D]."""
    R, W = qkv.shape[0], H * D
    pl = torch.as_tensor(pos, device=qkv.device).long()[:, None]
    heads = lambda t: t.float().view(R, 1, H, D).transpose(1, 2)
    qr, qe = rope_bf16(heads(qkv[:, :W]), pl, cos, sin)
    kr, ke = rope_bf16(heads(qkv[:, W:2 * W]), pl, cos, sin)
    return qr[:, :, 0], qe[:, :, 0], kr[:, :, 0], ke[:, :, 0]


def split_t_cap(chunk):
    return 2 * chunk + 37


def split_lens(chunk):
    """kv_len of the split grid: one key, around one chunk, two chunks, one past, and T_cap (not a multiple of 64)."""
    return [1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, split_t_cap(chunk)]


def split_seed(D, chunk):
    return 9100 + 10 * D + chunk // 128


def split_launches(chunk):
    """[(variant, kv_len, pos)] of the split grid (per-row state: pos[b] is row b's rotary position and cache row).  "edge":
    pos = kv_len - 1, the seven lengths in two launches.  "past": the form tests/test_split_rows_gpu.py defines -- the new row
    lies at or past kv_len (written, not attended), in the last attended chunk (rows 0 and 3) or in a chunk none of the row's keys
    is in (row 2); row 1 stays an edge row."""
    ls = split_lens(chunk)
    return [("edge", ls[:4], [n - 1 for n in ls[:4]]), ("edge", ls[4:], [n - 1 for n in ls[4:]]),
            ("past", ls[:4], [ls[0] + 3, ls[1] - 1, 2 * chunk + 3, ls[3] + 3])]


SPLIT_HEADS = 2
DRAFT_HEADS = 2


def draft_p0(K):
    """First positions of the draft grid, two launches of three groups: rows whose keys all come from the LDS copies (0), from
    both in one 128-key pass (1, 15, 120, 127: the pass edge falls inside the K rows for K = 8) and from the cache's end."""
    return [[0, 1, 15], [120, 127, DECODE_T - K]]


def draft_seed(D, K):
    return 11000 + 10 * D + K


# ---------------------------------------------------------------------------------------------------------------- shared
def rnd(*shape, seed, scale=1.0):
    """Seeded N(0, scale^2) fp32 on the host."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rope_tables(D, max_pos=512, device="cpu"):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(max_pos).float(), inv)
    return fr.cos().contiguous().to(device), fr.sin().contiguous().to(device)


class lib_options:
    """Set library options (include/myriad_hip.h mh_set_option) for a block; the previous values come back in any case."""

    def __init__(self, **opts):
        self.opts, self.prev = opts, {}

    def __enter__(self):
        from myriad_amd import _lib
        for k, v in self.opts.items():
            self.prev[k] = _lib.load().mh_set_option(k.encode(), int(v))
            assert self.prev[k] in (0, 1), k
        return self

    def __exit__(self, *exc):
        from myriad_amd import _lib
        for k, v in self.prev.items():
            _lib.load().mh_set_option(k.encode(), int(v))


# ---------------------------------------------------------------------------------------------------------------- row kernels
C_FN = 4.0                 # assumed ulp allowance of expf / logf / rsqrtf / sqrtf / a division (see the module docstring)
F32_TINY = 2.0 ** -126


def g_sum(n_thread: int, n_waves: int = 4) -> float:
    return (n_thread + 6 + n_waves + 4) * U32


def g_row(D: int) -> float:
    return g_sum(4 * -(-D // 1024), 4)


def f32_value(v: float) -> float:
    """The fp32 value a launcher's float argument takes."""
    return float(torch.tensor(v, dtype=torch.float32))


def _rel_rsqrt(rho):
    rho = rho.clamp(max=0.5)
    return 0.5 * rho * (1 + 2 * rho) + (C_FN + 1) * U32


def bf16_out(ref, e):
    return e + U16 * (ref.abs() + e)


def norm_rows(M: int, D: int, seed: int) -> torch.Tensor:
    """fp32 [M, D] test rows, by row index mod 6: N(0,1); N(0,1) + 1e3; all zeros; constant 0.75; 1e-4 N(0,1); 1e4 N(0,1)
    (the last two adjacent: a small row next to a large one)."""
    x = rnd(M, D, seed=seed)
    k = torch.arange(M) % 6
    x[k == 1] += 1e3
    x[k == 2] = 0.0
    x[k == 3] = 0.75
    x[k == 4] *= 1e-4
    x[k == 5] *= 1e4
    return x


def norm_weight(D: int, seed: int) -> torch.Tensor:
    """A norm weight with a zero and negative entries."""
    w = 1 + 0.5 * rnd(D, seed=seed)
    w[0] = 0.0
    w[1] = -1.3
    w[D - 1] = -0.4
    return w


def rmsnorm_ref_bound(x, w, eps, dy=None, dres=None, dy_err=None):
    """fp64 RMSNorm of fp32 x [M, D]: dict y, y_bound (fp32 value), y_bf16_bound; with dy also dx, dx_bound, dx_bf16_bound.
    dy_err: an element-wise bound on an error dy itself carries (dx is linear in dy: it enters as r |w| e and
    |x| r^3 / D sum |x w| e)."""
    x, w = x.double(), w.double()
    D = x.shape[1]
    eps = f32_value(eps)
    v = (x * x).mean(1, keepdim=True) + eps
    r = v.rsqrt()
    rel_r = _rel_rsqrt(torch.full_like(v, g_row(D) + 2 * U32))
    y = w * x * r
    e = y.abs() * (rel_r + 3 * U32)
    out = dict(y=y, y_bound=e, y_bf16_bound=bf16_out(y, e))
    if dy is None:
        return out
    g = dy.double()
    t1 = r * w * g
    dot = (x * w * g).sum(1, keepdim=True)
    cc = r ** 3 * dot / D
    e_cc = r ** 3 / D * (g_row(D) + 2 * U32) * (x * w * g).abs().sum(1, keepdim=True) + (3 * rel_r + 4 * U32) * cc.abs()
    dx = t1 - x * cc
    if dres is not None:
        dx = dx + dres.double()
    e = (rel_r + 4 * U32) * t1.abs() + x.abs() * (e_cc + 2 * U32 * cc.abs()) + 2 * U32 * dx.abs()
    if dy_err is not None:
        de = dy_err.double()
        e = e + r * w.abs() * de + x.abs() * r ** 3 / D * ((x * w).abs() * de).sum(1, keepdim=True)
    out.update(dx=dx, dx_bound=e, dx_bf16_bound=bf16_out(dx, e))
    return out


def layernorm_ref_bound(x, w, b, eps, dy=None, dres=None, dy_err=None):
    """fp64 LayerNorm of fp32 x [M, D] (b may be None for the backward only): dict y, y_bound, y_bf16_bound; with dy also dx,
    dx_bound, dx_bf16_bound.  Raises if a row's variance is lost to the mean's rounding although the row is not constant.
    dy_err: an element-wise bound on an error dy itself carries.  dx = r (gw - mean(gw) - xh mean(gw xh)), gw = dy w, is linear in
    dy, so a dy moved by at most e moves it by at most r (|w| e + mean(|w| e) + |xh| mean(|w| e |xh|)); what the other terms of
    the bound change when they are evaluated at the moved dy is of the order u32 e and left out."""
    x, w = x.double(), w.double()
    D = x.shape[1]
    eps = f32_value(eps)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    r = (var + eps).rsqrt()
    e_mean = g_row(D) * x.abs().mean(1, keepdim=True) + U32 * mean.abs()
    rho = (e_mean ** 2 + (g_row(D) + 6 * U32) * var) / (var + eps)
    if not bool(((rho <= 0.5) | (d.abs().amax(1, keepdim=True) == 0)).all()):
        raise ValueError("layernorm_ref_bound: a non-constant row whose variance is below the mean's rounding error")
    rel_r = _rel_rsqrt(rho)
    xh = d * r
    e_xh = r * e_mean + xh.abs() * (rel_r + 2 * U32)
    out = dict(xhat=xh, xhat_bound=e_xh)
    if b is not None:
        y = d * r * w + b.double()
        e = (r * w).abs() * e_mean + (d * r * w).abs() * (rel_r + 4 * U32) + 2 * U32 * y.abs()
        out.update(y=y, y_bound=e, y_bf16_bound=bf16_out(y, e))
    if dy is None:
        return out
    gw = dy.double() * w
    sg = gw.mean(1, keepdim=True)
    sgx = (gw * xh).mean(1, keepdim=True)
    e_sg = (g_row(D) + 2 * U32) * gw.abs().mean(1, keepdim=True)
    e_sgx = (g_row(D) + 4 * U32) * (gw * xh).abs().mean(1, keepdim=True) + (gw.abs() * e_xh).mean(1, keepdim=True)
    inner = gw - sg - xh * sgx
    e_inner = e_sg + sgx.abs() * e_xh + xh.abs() * e_sgx + 4 * U32 * (gw.abs() + sg.abs() + (xh * sgx).abs())
    core = r * inner
    dr = dres.double() if dres is not None else torch.zeros_like(core)
    dx = core + dr
    e = r * e_inner + core.abs() * (rel_r + U32) + 2 * U32 * (dx.abs() + dr.abs())
    if dy_err is not None:
        we = w.abs() * dy_err.double()
        e = e + r * (we + we.mean(1, keepdim=True) + xh.abs() * (we * xh.abs()).mean(1, keepdim=True))
    out.update(dx=dx, dx_bound=e, dx_bf16_bound=bf16_out(dx, e))
    return out


def ln_dropout_fwd_ref_bound(z, res, w, b, eps, keep_in=None, keep_out=None, x_out=None):
    """fp64 references of mh_layernorm_fwd_dropout (module docstring): dict x, x_bound (res given: x = z keep_in + res) and y,
    y_bound, y_bf16_bound of y = LN(x_in) keep_out, where x_in is the fp32 x_out the kernel wrote and re-reads (res given) or
    z itself.  keep_* : [M, D] factors (0 or the fp32 quotient), None for p = 0."""
    z64 = z.double()
    out = {}
    x_in = z
    if res is not None:
        zk = z64 * keep_in.double() if keep_in is not None else z64
        x = zk + res.double()
        out.update(x=x, x_bound=2 * U32 * (zk.abs() + x.abs()))
        x_in = x_out
    r = layernorm_ref_bound(x_in, w, b, eps)
    y, e = r["y"], r["y_bound"]
    if keep_out is not None:
        ko = keep_out.double()
        y = y * ko
        e = ko * e + U32 * y.abs()
    out.update(y=y, y_bound=e, y_bf16_bound=bf16_out(y, e))
    return out


def ln_dropout_bwd_ref_bound(dy, x, w, eps, keep_in=None, keep_out=None):
    """fp64 references of mh_layernorm_bwd_dropout: g = dy keep_out (one fp32 product: dy_err = u32 |g|) through
    layernorm_ref_bound gives dx (the residual's gradient, unmasked) and dx_bound; dz = bf16(dx keep_in) with
    dz_bound = bf16_out(dz, keep_in e + u32 |dz|)."""
    g, ge = dy.double(), None
    if keep_out is not None:
        g = g * keep_out.double()
        ge = U32 * g.abs()
    r = layernorm_ref_bound(x, w, None, eps, dy=g, dy_err=ge)
    dx, e = r["dx"], r["dx_bound"]
    dz, ez = dx, e
    if keep_in is not None:
        ki = keep_in.double()
        dz = dx * ki
        ez = ki * e + U32 * dz.abs()
    return dict(dx=dx, dx_bound=e, dz=dz, dz_bound=bf16_out(dz, ez))


def ln_dropout_inputs(M: int, D: int, form: str, seed: int):
    """(z, res, w, b, dy, p_in, p_out) fp32 on the host for the four forms mh_layernorm_fwd_dropout is called in: "a" the
    embeddings form (no residual, output mask; z = norm_rows), "b" the sublayer form (res = norm_rows, z ~ N(0,1), input mask),
    "c" both masks, "d" a residual and no mask.  The weight has a zero and negative entries where D allows."""
    w = norm_weight(D, seed=seed + 2) if D >= 8 else 1 + 0.5 * rnd(D, seed=seed + 2)
    b, dy = 0.1 * rnd(D, seed=seed + 3), rnd(M, D, seed=seed + 4)
    if form == "a":
        return norm_rows(M, D, seed=seed), None, w, b, dy, 0.0, 0.1
    p_in, p_out = {"b": (0.1, 0.0), "c": (0.1, 0.5), "d": (0.0, 0.0)}[form]
    return rnd(M, D, seed=seed + 1), norm_rows(M, D, seed=seed), w, b, dy, p_in, p_out


TN_BM = 32                 # reduction rows one step of mh_gemm_tn_wgrad stages: one MFMA per step and output tile


def tn_rows_per(M: int, splits: int) -> int:
    """Rows a split of mh_gemm_tn_wgrad covers: ceil(M / splits) rounded up to whole 32-row steps (at least one)."""
    return max(TN_BM, -(-(-(-M // splits)) // TN_BM) * TN_BM)


def tn_wgrad_ref_bound(dy, x, splits, prev=None, prev_bias=None):
    """fp64 (dW, bound, db, bound) of mh_gemm_tn_wgrad: dW [N, K] = dy^T x (+ prev), db [N] = sum_m dy (+ prev_bias), from
    bf16 dy [M, N], x [M, K].  A split adds one 16x16x32 MFMA per 32-row step to its fp32 accumulator (32 exact bf16 products
    and one rounding each; g_acc counts two per 32) and the splits are summed in split order: g_acc(M, splits) |dy|^T |x|, and
    u32 |dW| for the sum onto prev.  db: a staging thread adds its column's value at every step of its split serially
    (rows_per / 32 terms), the 32 staging rows are added in order, then the splits:
    (ceil(rows_per / 32) + 32 + splits + 1) u32 sum_m |dy| (+ u32 |db| for the sum onto prev_bias)."""
    d64, x64 = dy.double(), x.double()
    M = d64.shape[0]
    dW = d64.T @ x64
    e_W = g_acc(M, splits) * (d64.abs().T @ x64.abs())
    db = d64.sum(0)
    e_b = (-(-tn_rows_per(M, splits) // TN_BM) + TN_BM + splits + 1) * U32 * d64.abs().sum(0)
    if prev is not None:
        dW = dW + prev.double()
        e_W = e_W + U32 * dW.abs()
    if prev_bias is not None:
        db = db + prev_bias.double()
        e_b = e_b + U32 * db.abs()
    return dW, e_W, db, e_b


LNP_ROWS = 16              # rows a partial block of mh_layernorm_param_grads sums serially


def layernorm_param_grads_ref_bound(dy, x, eps, keep=None, prev=None):
    """fp64 (dgamma, bound, dbeta, bound) of dgamma = sum_m g xhat, dbeta = sum_m g with g = dy * keep (keep: the dropout mask on
    the LayerNorm's output, or None) (+ prev = (dgamma0, dbeta0) for the accumulate form).  A column is summed serially over the
    16 rows of a block, then over the ceil(M/16) blocks: n = 16 + ceil(M/16) additions, + 3 for the products' roundings;
    xhat's own error (layernorm_ref_bound's e_xh, from the row statistics) enters weighted by |g|."""
    M, D = x.shape
    r = layernorm_ref_bound(x, torch.ones(D, dtype=torch.float64, device=x.device), None, eps)
    xh, e_xh = r["xhat"], r["xhat_bound"]
    g = dy.double() * (keep.double() if keep is not None else 1.0)
    n = (LNP_ROWS + -(-M // LNP_ROWS) + 3) * U32
    dg, db = (g * xh).sum(0), g.sum(0)
    e_g = (g.abs() * e_xh).sum(0) + n * (g * xh).abs().sum(0)
    e_b = n * g.abs().sum(0)
    if prev is not None:
        dg, db = dg + prev[0].double(), db + prev[1].double()
        e_g = e_g + U32 * dg.abs()
        e_b = e_b + U32 * db.abs()
    return dg, e_g, db, e_b


LR_CHUNKS = 16             # row chunks of the low-rank adaptor's weight-gradient partials


def lowrank_ref_bound(x, A, Bm, dy=None, t_in=None):
    """fp64 rank-R adaptor y = x + (x A^T) Bm^T (A [R, D], Bm [D, R], all fp32): dict t, t_bound, y, y_bound; with dy also dx, dA,
    dB and bounds, dB from the t it is handed (t_in, default the exact one).  The R dot products of a row are block sums of D
    terms (g_sum(ceil(D/256), 4) on |x||A|^T); the rank-R update is R serial FMAs; a weight-gradient column sums its chunk's rows
    in four interleaved serial sums, adds those, then the 16 chunks in order: (ceil(ceil(M/16)/4) + 3 + 16 + 2) u32 on the
    magnitudes |dt|^T |x| and |dy|^T |t| -- a gradient that cancels over the rows keeps the bound of its terms."""
    x, A, Bm = x.double(), A.double(), Bm.double()
    M, D = x.shape
    R = A.shape[0]
    gd = g_sum(-(-D // 256), 4)
    t = x @ A.T
    e_t = gd * (x.abs() @ A.abs().T)
    y = x + t @ Bm.T
    e_y = e_t @ Bm.abs().T + (R + 2) * U32 * (x.abs() + t.abs() @ Bm.abs().T)
    out = dict(t=t, t_bound=e_t, y=y, y_bound=e_y)
    if dy is None:
        return out
    g = dy.double()
    tt = t if t_in is None else t_in.double()
    dt = g @ Bm
    e_dt = gd * (g.abs() @ Bm.abs())
    dx = g + dt @ A
    e_dx = e_dt @ A.abs() + (R + 2) * U32 * (g.abs() + dt.abs() @ A.abs())
    n = (-(-(-(-M // LR_CHUNKS)) // 4) + 3 + LR_CHUNKS + 2) * U32
    dA = dt.T @ x
    e_dA = e_dt.T @ x.abs() + n * (dt.abs().T @ x.abs())
    dB = g.T @ tt
    e_dB = n * (g.abs().T @ tt.abs())
    out.update(dx=dx, dx_bound=e_dx, dA=dA, dA_bound=e_dA, dB=dB, dB_bound=e_dB)
    return out


def assert_rope_exempt_share(unc, what=""):
    """The condition on rope_bf16's uncertainty mask: at most 1 % of the elements carry any, and no whole head row does."""
    amb = unc > 0
    share = float(amb.double().mean())
    assert share <= 0.01, f"{what}: {share:.3%} of the rotated elements are ambiguous"
    assert not bool(amb.all(-1).any()), f"{what}: a whole row is ambiguous"


def l2norm_ref_bound(x, eps):
    x = x.double()
    D = x.shape[1]
    n = (x * x).sum(1, keepdim=True).sqrt().clamp_min(f32_value(eps))
    y = x / n
    e = y.abs() * (g_row(D) / 2 + (2 * C_FN + 2) * U32)
    return y, e, bf16_out(y, e)


def sum_ref_bound(x, scale=1.0):
    x = x.double().reshape(-1)
    ref = x.sum() * f32_value(scale)
    return ref, abs(f32_value(scale)) * g_sum(-(-x.numel() // 256), 4) * x.abs().sum() + U32 * ref.abs()


CE_LO = f32_value(1e-7)
CE_HI = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-7, dtype=torch.float32))


def clamp_ce_ref_bound(logits, labels, gscale, ldd=None, n_thread=None, n_waves=16):
    """fp64 clamp-CE of fp32 logits [R, V] (-inf allowed) and labels [R] (-100 / out of range: no label).  Returns a dict:
    loss, loss_bound [R]; dlog, dlog_bound [R, ldd] (bf16 output, pad columns exactly 0); amb [R]: rows whose p_t is within its
    bound of a clamp threshold -- for these loss_alt / dlog_alt hold the other branch.  n_thread / n_waves: the kernel's
    summation shape (default covers both kernels: max(32, ceil(V/256)) terms a thread, 16 waves)."""
    x = logits.double()
    R, V = x.shape
    ldd = V if ldd is None else ldd
    gs = f32_value(gscale)
    n_thread = max(32, -(-V // 256)) if n_thread is None else n_thread
    m = x.amax(1, keepdim=True)
    a = x - m
    ex = a.exp()
    se = ex.sum(1, keepdim=True)
    p = ex / se
    absa = torch.where(p > 0, a.abs(), torch.zeros_like(a))
    rel_se = g_sum(n_thread, n_waves) + U32 * (p * (C_FN + 1 + absa)).sum(1, keepdim=True)
    rho = rel_se + (C_FN + 4 + absa) * U32
    t = labels.long()
    has = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)[:, None]
    pt, rho_t = p.gather(1, tc)[:, 0], rho.gather(1, tc)[:, 0]
    slack = rho_t * pt
    # p_t = 1 in fp32 for certain: the label's logit is the maximum (exp(0) = 1) and everything else sums to less than half an
    # ulp of 1, so every partial sum that holds the 1 rounds back to 1 whatever the order, 1 / 1 = 1 and the row is saturated
    a_t = a.gather(1, tc)[:, 0]
    sure_one = (a_t == 0) & ((se[:, 0] - 1) * 1.001 < U32 / 2)
    amb = has & (((pt - CE_LO).abs() <= slack) | (((pt - CE_HI).abs() <= slack + 2 * U32) & ~sure_one))
    inside = (pt >= CE_LO) & (pt <= CE_HI)
    onehot = torch.zeros_like(p).scatter_(1, tc, 1.0)
    g_in = gs * (p - onehot)
    e_in = abs(gs) * (rho * p + U32 * (p - onehot).abs()) + U32 * g_in.abs()
    e_in = bf16_out(g_in, e_in)
    loss_in = -pt.clamp(CE_LO, CE_HI).log()
    loss_in_b = rho_t + (C_FN + 1) * U32 * loss_in.abs()
    # the other side of the nearest threshold
    near_lo = (pt - CE_LO).abs() <= (pt - CE_HI).abs()
    loss_out = -torch.where(near_lo, torch.full_like(pt, CE_LO), torch.full_like(pt, CE_HI)).log()
    loss_out_b = (C_FN + 1) * U32 * loss_out.abs()

    def pick(cond, a_, b_):
        return torch.where(cond if a_.dim() == 1 else cond[:, None], a_, b_)

    zero = torch.zeros_like(g_in)
    live = has & inside
    dlog = pick(live, g_in, zero)
    dlog_b = pick(live, e_in, zero)
    dlog_alt = pick(has & ~inside, g_in, zero)
    dlog_alt_b = pick(has & ~inside, e_in, zero)
    z1 = torch.zeros_like(pt)
    loss = pick(has, pick(inside, loss_in, loss_out), z1)
    loss_b = pick(has, pick(inside, loss_in_b, loss_out_b), z1)
    # the clamp is continuous in p_t: either branch's loss is within the other's bound of the threshold value
    loss_alt, loss_alt_b = loss, loss_b + loss_in_b

    def pad(v):
        return torch.nn.functional.pad(v, (0, ldd - V))

    return dict(loss=loss, loss_bound=loss_b, dlog=pad(dlog), dlog_bound=pad(dlog_b), amb=amb, loss_alt=loss_alt,
                loss_alt_bound=loss_alt_b, dlog_alt=pad(dlog_alt), dlog_alt_bound=pad(dlog_alt_b), p=p, has=has, inside=inside)


def clamp_ce_check(row_loss, dlog, r, what="clamp_ce"):
    """Assert row_loss [R] and dlog [R, ldd] (or None) against clamp_ce_ref_bound's dict; a threshold row may take either
    branch.  Returns (worst loss ratio, worst dlogits ratio) over the unambiguous rows."""
    amb = r["amb"]
    keep = ~amb
    w_loss = assert_within(row_loss[keep], r["loss"][keep], r["loss_bound"][keep], what + " row_loss")
    w_d = 0.0
    if dlog is not None:
        w_d = assert_within(dlog[keep], r["dlog"][keep], r["dlog_bound"][keep], what + " dlogits")
    for i in amb.nonzero()[:, 0].tolist():
        errs = []
        for sfx in ("", "_alt"):
            try:
                assert_within(row_loss[i:i + 1], r["loss" + sfx][i:i + 1], r["loss" + sfx + "_bound"][i:i + 1], f"{what} row {i} loss")
                if dlog is not None:
                    assert_within(dlog[i], r["dlog" + sfx][i], r["dlog" + sfx + "_bound"][i], f"{what} row {i} dlogits")
                break
            except AssertionError as e:
                errs.append(str(e))
        else:
            raise AssertionError(f"{what}: threshold row {i} matches neither branch: " + " | ".join(errs))
    return w_loss, w_d


def ce_case(R: int, V: int, seed: int):
    """Logits [R, V] (R >= 10) and labels for the clamp-CE edge rows: 0 label 0; 1 label V-1; 2 a label in the last partial
    float4 (or V-2); 3 no label (-100); 4 label >= V; 5 a -inf logit elsewhere; 6 the label's own logit -inf; 7 p_t far below
    1e-7; 8 p_t far above 1 - 1e-7; the rest random labels."""
    x = rnd(R, V, seed=seed) * 2
    g = torch.Generator().manual_seed(seed + 1)
    y = torch.randint(0, V, (R,), generator=g)
    y[0], y[1], y[2], y[3], y[4] = 0, V - 1, (V // 4) * 4 if V % 4 else V - 2, -100, V + 3
    x[5, (int(y[5]) + 7) % V] = float("-inf")
    x[5, V - 1 if int(y[5]) != V - 1 else V - 2] = float("-inf")
    x[6, y[6]] = float("-inf")
    x[7, y[7]] = x[7].min() - 30
    x[8, y[8]] = x[8].max() + 40
    return x, y


def argmax_ref(x, ban_id=-1, inv_temp=1.0):
    """(ids, margin, margin bound, p_max, p_max relative bound) in fp64; ids: first index on ties, the banned id counts as -inf."""
    x = x.double().clone()
    if ban_id >= 0:
        x[:, ban_id] = float("-inf")
    ids = x.argmax(1)                                   # torch: first index on ties
    top = x.topk(2, 1).values
    margin = top[:, 0] - top[:, 1]
    a = (x - top[:, :1]) * f32_value(inv_temp)
    ex = a.exp()
    s = ex.sum(1)
    p = ex / s[:, None]
    absa = torch.where(p > 0, a.abs(), torch.zeros_like(a))
    rel = max(g_sum(32, 16), g_sum(-(-x.shape[1] // 256), 4)) + U32 * (p * (4 + 2 * absa)).sum(1) + (C_FN + 1) * U32
    return ids, margin, U32 * margin.abs(), 1.0 / s, rel / s


# ---------------------------------------------------------------------------------------------------------------- elementwise
def _sigmoid_rel(g):
    s = torch.sigmoid(g)
    return s, (4 + 2 * g.abs()) * U32 * (1 - s) + 3 * U32


def silu_mul_ref_bound(g, u, dh=None):
    """fp64 h = silu(g) u of bf16-valued g, u (bound incl. the bf16 output rounding); with dh also (dg, bound), (du, bound)."""
    g, u = g.double(), u.double()
    s, rel_s = _sigmoid_rel(g)
    h = g * s * u
    out = [h, bf16_out(h, h.abs() * (rel_s + 3 * U32) + F32_TINY)]
    if dh is None:
        return out
    d = dh.double()
    f = s + g * s * (1 - s)
    e_f = (s * rel_s + g.abs() * s * (1 - s) * (rel_s + 2 * U32) + g.abs() * s * (s * rel_s + U32)
           + U32 * (f.abs() + (g * s * (1 - s)).abs()))
    dg = d * u * f
    du = d * g * s
    out += [dg, bf16_out(dg, (d * u).abs() * e_f + 3 * U32 * dg.abs() + F32_TINY),
            du, bf16_out(du, du.abs() * (rel_s + 3 * U32) + F32_TINY)]
    return out


def gelu_ref_bound(x, dy=None):
    """fp64 erf-GELU of bf16-valued x (bf16 output); with dy the backward dy gelu'(x) instead."""
    x = x.double()
    cdf = 0.5 * torch.special.erfc(-x / 2 ** 0.5)
    if dy is None:
        y = x * cdf
        return y, bf16_out(y, 4 * U32 * y.abs() + 2e-7 * x.abs() + F32_TINY)
    pdf = torch.exp(-x * x / 2) * 0.39894228040143267794
    gp = cdf + x * pdf
    ref = dy.double() * gp
    e = dy.double().abs() * (2e-7 + (x * pdf).abs() * (4 + x * x) * U32 + 4 * U32 * gp.abs()) + U32 * ref.abs() + F32_TINY
    return ref, bf16_out(ref, e)


def rope_rows_ref(x2d, col0, n_heads, head_dim, pos, cos, sin, sign=1.0):
    """rope_bf16 for the in-place layout: x2d [n_tok, ld] bf16, heads at col0.  Returns (ref, ambiguity) as [n_tok, nh * d]."""
    n = x2d.shape[0]
    xs = x2d[:, col0:col0 + n_heads * head_dim].float().reshape(1, n, n_heads, head_dim).transpose(1, 2)
    rb, amb = rope_bf16(xs, pos.long().reshape(1, n), cos, sin, sign)
    return rb.transpose(1, 2).reshape(n, -1), amb.transpose(1, 2).reshape(n, -1)


EW_WRAP = 2 * 4096 * 256      # items a 4096 x 256 elementwise grid covers in two sweeps: more than this needs a third


def frame_of(buf, win_rows: slice, win_cols: slice):
    """The parts of a 2-D (or [.., rows, cols]) buffer outside the window, as a list of views."""
    r0, r1, c0, c1 = win_rows.start, win_rows.stop, win_cols.start, win_cols.stop
    return [buf[..., :r0, :], buf[..., r1:, :], buf[..., r0:r1, :c0], buf[..., r0:r1, c1:]]


def assert_frame_untouched(buf, win_rows: slice, win_cols: slice, what=""):
    for i, f in enumerate(frame_of(buf, win_rows, win_cols)):
        assert_untouched(f, f"{what} frame part {i}")


def out_window(B, S, W, device):
    """A poisoned bf16 [B, S, W] view of a [B, S + 4, W + 8] buffer (the extra rows and columns must stay untouched)."""
    buf = poisoned((B, S + 4, W + 8), torch.bfloat16, device)
    return buf, buf[:, :S, :W]


def check_outside(buf, S, W, what):
    assert_untouched(buf[:, S:], what + " rows past S")
    assert_untouched(buf[:, :, W:], what + " columns past W")


# ---------------------------------------------------------------------------------------------------------------- conv stack
def conv_out_hw(H, W, kh, kw, pad):
    return H + 2 * pad - kh + 1, W + 2 * pad - kw + 1


def im2col_ref(x, kh, kw, pad, Kpad, bias_col):
    """[B*OH*OW, Kpad] in x's dtype from x [B, H, W, C]: column (ky*kw + kx)*C + c of row (b, oy, ox) is x[b, oy+ky-pad, ox+kx-pad, c],
    0 outside the image; column K is 1 with bias_col; every other column >= K is 0."""
    B, H, W, C = x.shape
    OH, OW = conv_out_hw(H, W, kh, kw, pad)
    K = kh * kw * C
    xp = torch.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype=x.dtype, device=x.device)
    xp[:, pad:pad + H, pad:pad + W] = x
    col = torch.zeros((B, OH, OW, Kpad), dtype=x.dtype, device=x.device)
    for ky in range(kh):
        for kx in range(kw):
            t = ky * kw + kx
            col[..., t * C:(t + 1) * C] = xp[:, ky:ky + OH, kx:kx + OW]
    if bias_col:
        col[..., K] = 1.0
    return col.view(B * OH * OW, Kpad)


def col2im_fold(t, B, H, W, C, kh, kw, pad):
    """The fp64 transpose of im2col_ref: [B, H, W, C] with out[b, y, x, c] = sum_taps t[(b, y+pad-ky, x+pad-kx), tap*C + c] (t [M, ld],
    only its first kh*kw*C columns are read)."""
    OH, OW = conv_out_hw(H, W, kh, kw, pad)
    t = t.double().reshape(B, OH, OW, -1)
    out = torch.zeros((B, H + 2 * pad, W + 2 * pad, C), dtype=torch.float64, device=t.device)
    for ky in range(kh):
        for kx in range(kw):
            k0 = (ky * kw + kx) * C
            out[:, ky:ky + OH, kx:kx + OW] += t[..., k0:k0 + C]
    return out[:, pad:pad + H, pad:pad + W]


def col2im_ref_bound(dcol, B, H, W, C, kh, kw, pad):
    return col2im_fold(dcol, B, H, W, C, kh, kw, pad), kh * kw * U32 * col2im_fold(dcol.double().abs(), B, H, W, C, kh, kw, pad)


def pool_windows(y2d, B, H, W, C):
    """[B, H/2, W/2, C, 4] view-copy of y2d [B*H*W, >= C]: the 2x2 windows in the order (0,0), (0,1), (1,0), (1,1)."""
    return y2d[:, :C].reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def _pool_values(y2d):
    return y2d.float() if y2d.dtype == torch.bfloat16 else y2d               # bf16 -> fp32 is exact; fp32 / fp64 stay as they are


def relu_pool_fwd_ref(y2d, B, H, W, C):
    return pool_windows(_pool_values(y2d), B, H, W, C).amax(-1).clamp_min(0.0).to(torch.bfloat16)


def relu_pool_bwd_ref(dp, y2d, B, H, W, C, cpad=None):
    """dy [B*H*W, cpad] bf16: bf16(dp) at the first maximum of each window iff that maximum is > 0, zero elsewhere."""
    cpad = C if cpad is None else cpad
    w = pool_windows(_pool_values(y2d), B, H, W, C)
    arg = w.argmax(-1, keepdim=True)                                       # torch: the first index on ties
    g = torch.where(w.amax(-1) > 0, dp.reshape(B, H // 2, W // 2, C).to(torch.bfloat16), torch.zeros((), dtype=torch.bfloat16, device=dp.device))
    d4 = torch.zeros(w.shape, dtype=torch.bfloat16, device=dp.device).scatter_(-1, arg, g[..., None])
    dy = d4.reshape(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B * H * W, C)
    return torch.nn.functional.pad(dy, (0, cpad - C))


def pool_edge_windows(B, H, W, C, seed, dtype=torch.float32):
    """y [B*H*W, C] in `dtype` (values exact in it) with twelve constructed windows in a row (in the flat [B, H/2, W/2, C] window order),
    repeated at up to 64 places spread over the images, rows and channels: all four equal and positive; the six two-way ties; all negative; maximum exactly 0.0; maximum -0.0; a maximum one
    ulp of `dtype` above the runner-up -- in fp32 far below bf16's resolution -- once with the runner-up first and once with the
    maximum first and last; the rest random.  Needs B (H/2) (W/2) C >= 12 windows."""
    y = rnd(B * H * W, C, seed=seed).to(dtype).float()
    w = pool_windows(y, B, H, W, C).reshape(-1, 4).clone()
    n = w.shape[0]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    rows = []
    rows.append([0.75, 0.75, 0.75, 0.75])
    for a, b in pairs:
        r = [-0.5, 0.25, -1.0, 0.125]
        r[a] = r[b] = 1.5
        rows.append(r)
    rows.append([-0.5, -2.0, -0.25, -1.0])
    rows.append([-1.0, 0.0, -0.5, -3.0])
    rows.append([-1.0, -2.0, -0.0, -0.5])
    one = torch.tensor(1.0, dtype=dtype)
    up = float(torch.nextafter(one, one * 2)) if dtype == torch.float32 else 1.0 + 2.0 ** -7
    rows.append([1.0, 0.5, up, 1.0])
    rows.append([up, 1.0, 1.0, up])
    pat = torch.tensor(rows, dtype=torch.float32)
    reps = min(n // pat.shape[0], 64)
    stride = max(1, n // max(reps, 1))
    for r in range(reps):                                                      # spread over images, rows and channels
        i0 = r * stride
        if i0 + pat.shape[0] <= n:
            w[i0:i0 + pat.shape[0]] = pat
    y = w.reshape(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B * H * W, C)
    return y.to(dtype)


def conv_pack_ref(Wm, bias, Kpad):
    Cout, K = Wm.shape
    out = torch.zeros((Cout, Kpad), dtype=torch.bfloat16, device=Wm.device)
    out[:, :K] = Wm.to(torch.bfloat16)
    if bias is not None:
        out[:, K] = bias.to(torch.bfloat16)
    return out


def pool_decisions(y64, e_y, B, H, W, C):
    """Windows [B, H/2, W/2, C] (bool) of a conv pre-activation y64 [B*H*W, C] known to within e_y whose pooling is a decision:
    the runner-up lies within the two bounds of the maximum, or the maximum lies within its bound of 0."""
    w, e = pool_windows(y64, B, H, W, C), pool_windows(e_y, B, H, W, C)
    top, arg = w.max(-1, keepdim=True)
    e_top = e.gather(-1, arg)
    other = torch.ones_like(w, dtype=torch.bool).scatter_(-1, arg, False)
    close = (other & (w + e >= top - e_top)).any(-1)
    return close | (top[..., 0].abs() <= e_top[..., 0])


# ---------------------------------------------------------------------------------------------------------------- map heads
def pair_logits_ref_bound(p, text, rows_per_batch, scale):
    """fp64 [rows, 2] = scale <p, t_j> / ||p|| of fp32 p [rows, C] and text [B, 2, C], row r against pair r // rows_per_batch."""
    p64 = p.double()
    rows, C = p64.shape
    t = text.double()[torch.arange(rows, device=p.device) // rows_per_batch]          # [rows, 2, C]
    dot = (p64[:, None] * t).sum(-1)
    mag = (p64[:, None] * t).abs().sum(-1)
    n = (p64 * p64).sum(1, keepdim=True).sqrt()
    s = f32_value(scale)
    ref = s * dot / n
    g = g_sum(4 * -(-C // 256), 0)
    return ref, abs(s) / n * g * mag + ref.abs() * (g / 2 + (2 * C_FN + 2) * U32)


def _ac_axis(n_in, n_out, device):
    """align_corners=True source positions of n_out samples over n_in cells: (pos, i0, i1, t) with pos = o (n_in-1)/(n_out-1)."""
    o = torch.arange(n_out, dtype=torch.float64, device=device)
    pos = o * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros_like(o)
    i0 = pos.floor().long().clamp(max=max(n_in - 2, 0))
    return pos, i0, i0 + (1 if n_in > 1 else 0), pos - i0


def _nbr_max(s):
    """Max of s [B, a, b] over the 3 x 3 neighbourhood (a or b may be 0: returned as is)."""
    if s.numel() == 0:
        return s
    return torch.nn.functional.max_pool2d(s[:, None], 3, stride=1, padding=1)[:, 0]


def bilinear_ref_bound(x, H, W, one_minus=False, extra_rel=0.0):
    """fp64 align_corners=True resize of x [B, h, w] to [B, H, W] and its bound (module docstring); extra_rel: a relative error the
    input values themselves carry (zs_accumulate's rounded difference)."""
    x = x.double()
    B, h, w = x.shape
    py, y0, y1, ty = _ac_axis(h, H, x.device)
    px, x0, x1, tx = _ac_axis(w, W, x.device)
    ty, tx = ty[None, :, None], tx[None, None, :]

    def lerp(a):
        a00, a01 = a[:, y0][:, :, x0], a[:, y0][:, :, x1]
        a10, a11 = a[:, y1][:, :, x0], a[:, y1][:, :, x1]
        return (1 - ty) * ((1 - tx) * a00 + tx * a01) + ty * ((1 - tx) * a10 + tx * a11)

    v, mag = lerp(x), lerp(x.abs())
    e = (6 * U32 + extra_rel) * mag
    if h > 1:                                                   # slope along y of cell row i, at every column; 3 x 3 neighbourhood
        sy = _nbr_max((x[:, 1:] - x[:, :-1]).abs())
        slope = torch.maximum(sy[:, y0][:, :, x0], sy[:, y0][:, :, x1])
        e = e + 2 * U32 * py[None, :, None] * slope
    if w > 1:
        sx = _nbr_max((x[:, :, 1:] - x[:, :, :-1]).abs())
        slope = torch.maximum(sx[:, y0][:, :, x0], sx[:, y1][:, :, x0])
        e = e + 2 * U32 * px[None, None, :] * slope
    if one_minus:
        v = 1 - v
        e = e + U32 * v.abs()
    return v, e


def _sigmoid_through(d, e_d):
    """(sigmoid(d), absolute bound) for the kernel's 1 / (1 + __expf(-d')) with |d' - d| <= e_d."""
    s, rel = _sigmoid_rel(d)
    slope = (s * (1 - s) * torch.exp(e_d)).clamp(max=0.25)
    return s, slope * e_d + s * rel + F32_TINY


def zs_accumulate_ref_bound(logits, mask_prev, map_prev, w):
    """fp64 (mask, mask bound, map, map bound) after mask_prev [B, h, h] += w sigmoid(l1 - l0), map_prev [B, S, S] +=
    w sigmoid(bilinear_ac(l1 - l0)) for fp32 logits [B, h*h, 2]."""
    B, h, S = mask_prev.shape[0], mask_prev.shape[-1], map_prev.shape[-1]
    w = f32_value(w)
    d = (logits.double()[..., 1] - logits.double()[..., 0]).reshape(B, h, h)
    s, e_s = _sigmoid_through(d, U32 * d.abs())
    mask = mask_prev.double() + w * s
    e_mask = abs(w) * e_s + U32 * (mask_prev.double().abs() + (w * s).abs())
    di, e_di = bilinear_ref_bound(d, S, S, extra_rel=U32)
    si, e_si = _sigmoid_through(di, e_di)
    amap = map_prev.double() + w * si
    e_map = abs(w) * e_si + U32 * (map_prev.double().abs() + (w * si).abs())
    return mask, e_mask, amap, e_map


def rowmax_skip_ref_bound(s, acc_prev, period, w):
    """fp64 acc_prev[row] + w max_{c % period != 0} s[row, c] (period <= 0: every column) and its bound; -inf where no finite
    column is kept (compare those rows with rowmax_check)."""
    s = s.double()
    w = f32_value(w)
    c = torch.arange(s.shape[1], device=s.device)
    keep = (c % period != 0) if period > 0 else torch.ones_like(c, dtype=torch.bool)
    m = s.masked_fill(~keep[None], float("-inf")).amax(1) if bool(keep.any()) else torch.full_like(s[:, 0], float("-inf"))
    ref = acc_prev.double() + w * m
    return ref, 2 * U32 * (acc_prev.double().abs() + (w * m).abs())


def rowmax_check(got, ref, bound, what="rowmax_skip"):
    """assert_within where the reference is finite; an infinite reference must be met exactly."""
    inf = torch.isinf(ref)
    assert torch.equal(got.double()[inf], ref[inf]), f"{what}: a row without a finite kept column is not {ref[inf][:1].tolist()}"
    return assert_within(got[~inf], ref[~inf], bound[~inf], what)


# ---------------------------------------------------------------------------------------------------------------- stem chain
CHAIN_CASES = [(1, 4, 2, 32, 32, 901), (4, 16, 2, 16, 24, 902)]            # ci, co, B, H, W, seed: VENet's first two stem layers


def stem_chain_case(ci, co, B, H, W, seed):
    """(x [B, H, W, ci] bf16, wm [co, 9 ci] f32 in GEMM order, bias [co] f32, dp [B, H/2, W/2, co] f32 with bf16 values)."""
    return (rnd(B, H, W, ci, seed=seed).to(torch.bfloat16), rnd(co, 9 * ci, seed=seed + 1) * 0.3, rnd(co, seed=seed + 2) * 0.1,
            bf16_round(rnd(B, H // 2, W // 2, co, seed=seed + 3)))


def stem_chain_ref(x, wm, bias, dp, wgrad_splits=1):
    """One stem layer in fp64 -- conv2d(3x3, pad 1) -> relu -> max_pool2d(2) and its autograd -- on the operands the kernels
    multiply (bf16 x, bf16-rounded weight and bias), with the bounds composed from gemm_ref_bound, the pooling's decisions and
    col2im's fold.  Windows whose routing is a decision (pool_decisions) get no gradient: dp_used is dp with those zeroed.
    Returns a dict (all [rows, cols] in the kernels' layouts)."""
    F = torch.nn.functional
    B, H, W, ci = x.shape
    co, K = wm.shape
    Kpad = (K + 1 + 63) // 64 * 64
    M = B * H * W
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = bf16_round(wm).double().reshape(co, 3, 3, ci).permute(0, 3, 1, 2).clone().requires_grad_(True)
    br = bf16_round(bias).double().clone().requires_grad_(True)
    y = F.conv2d(xr, wr, br, padding=1)
    y2d = y.detach().permute(0, 2, 3, 1).reshape(M, co)
    col, wp = im2col_ref(x, 3, 3, 1, Kpad, True), conv_pack_ref(wm, bias, Kpad)
    y_gemm, e_y = gemm_ref_bound(col, wp)
    dec = pool_decisions(y2d, e_y, B, H, W, co)
    dp_used = torch.where(dec, torch.zeros_like(dp), dp)
    pool = F.max_pool2d(F.relu(y), 2)
    (pool * dp_used.double().permute(0, 3, 1, 2)).sum().backward()
    e_p = pool_windows(e_y, B, H, W, co).amax(-1)
    p_ref = pool.detach().permute(0, 2, 3, 1)
    dy = relu_pool_bwd_ref(dp_used, y2d, B, H, W, co, 64)                                  # [M, 64] bf16, exact
    Mpad = (M + 63) // 64 * 64
    dyT = F.pad(dy[:, :co].T, (0, Mpad - M))
    colT = F.pad(col.T, (0, Mpad - M))
    dwp, e_dwp = gemm_ref_bound(dyT, colT, splits=wgrad_splits)
    wpT = F.pad(wp.T, (0, 64 - co))                                                         # [Kpad, 64]
    dcol, e_dcol = gemm_ref_bound(dy, wpT, out_bf16=True)
    dx = xr.grad.permute(0, 2, 3, 1)
    e_dx = col2im_fold(e_dcol, B, H, W, ci, 3, 3, 1) + 9 * U32 * col2im_fold(dcol.abs() + e_dcol, B, H, W, ci, 3, 3, 1)
    return dict(col=col, wp=wp, y=y2d, y_gemm=y_gemm, y_bound=e_y, decisions=dec, dp_used=dp_used, p=p_ref, p_bound=bf16_out(p_ref, e_p),
                dy=dy, dwp=dwp, dwp_bound=e_dwp, dW=wr.grad.permute(0, 2, 3, 1).reshape(co, K), db=br.grad, dcol=dcol,
                dcol_bound=e_dcol, dx=dx, dx_bound=e_dx, dx_fold=col2im_fold(dcol, B, H, W, ci, 3, 3, 1), K=K, Kpad=Kpad)


# ---------------------------------------------------------------------------------------------------------------- inputs
BF16 = torch.bfloat16


def col2im_input(B, H, W, C, kh, kw, pad, seed, device="cpu"):
    """A random bf16 dcol [M, Kpad] whose bias and pad columns hold large values (a tap that reads them shows)."""
    OH, OW = conv_out_hw(H, W, kh, kw, pad)
    K = kh * kw * C
    Kpad = (K + 64) // 64 * 64
    d = rnd(B * OH * OW, Kpad, seed=seed).to(BF16)
    d[:, K:] = 1e4
    return d.to(device)


def pair_inputs(rows, C, rpb, seed):
    """p [rows, C] with rows scaled by 1e-4 and 1e4 next to each other (row % 3 == 1, 2) and the text pairs [ceil(rows/rpb), 2, C]."""
    p = rnd(rows, C, seed=seed)
    k = torch.arange(rows) % 3
    p[k == 1] *= 1e-4
    p[k == 2] *= 1e4
    text = rnd(-(-rows // rpb), 2, C, seed=seed + 1)
    return p, text / text.norm(dim=-1, keepdim=True)


def zs_inputs(B, h, S, seed):
    """Logits [B, h*h, 2] whose differences reach +-60, and non-zero accumulators."""
    lg = rnd(B, h * h, 2, seed=seed) * 3
    lg[:, 0::5, 1] += torch.linspace(-60, 60, lg[:, 0::5].shape[1])[None]
    return lg, rnd(B, h, h, seed=seed + 1).abs(), rnd(B, S, S, seed=seed + 2).abs()


def rowmax_inputs(rows, cols, wide, seed):
    """scores [rows, cols] as a window of a [rows, wide] matrix whose excluded columns hold the row's largest values; row 0's
    maximum sits in column 0, row 1's in the last column, row 2 is -inf but for one entry, row 3's maximum sits in a multiple-of-5 column; and a non-zero accumulator."""
    full = rnd(rows, wide, seed=seed)
    full[:, cols:] = 50.0
    full[0, 0] = 9.0
    if rows > 1:
        full[1, cols - 1] = 8.0
    if rows > 2:
        full[2, :cols] = float("-inf")
        full[2, cols // 2] = -1.5
    if rows > 3:
        full[3, (cols - 1) // 5 * 5] = 9.5                   # a multiple of 5: skipped at period 5
    return full, rnd(rows, seed=seed + 1)


# ---------------------------------------------------------------------------------------------------------------- LoRA
LORA_BORDER = 64
LORA_V_TAG = 1 << 63
LORA_DOWN_WAVES = 8        # waves of a lora_down workgroup: each sums its own k-steps, the partial sums are added like slabs
LORA_WG_CHUNKS = 64        # row chunks of the thread-per-column weight-gradient kernel
LORA_WG_MFMA_CHUNKS = 16   # row chunks of the MFMA weight-gradient kernel


def keep_mask_ref(seed, M, D, p, second=False):
    """The dropout keep mask [M, D] fp32 of csrc/common.h restated in integer arithmetic (numpy uint64, masked to 32 bits after
    every product): element (m, d) hashes the flat index m D + d with the seed's low 63 bits; second (or bit 63 of the seed) takes
    dropout_hash2 of that hash.  u = (h >> 8) 2^-24 (exact in fp32); kept iff float32(u) >= float32(p); the value is the fp32
    quotient 1 / (1 - p), and 1.0 everywhere for p == 0."""
    import numpy as np
    p32 = np.float32(p)
    if not p32 > 0:
        return torch.ones(M, D, dtype=torch.float32)
    seed = int(seed)
    second = bool(second) or bool((seed >> 63) & 1)
    m32 = np.uint64(0xFFFFFFFF)
    idx = np.arange(M * D, dtype=np.uint64)
    lo, hi = idx & m32, idx >> np.uint64(32)
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0x7FFFFFFF)
    h = (lo * np.uint64(0x9E3779B1) + (s_lo ^ ((hi * np.uint64(0x85EBCA77)) & m32))) & m32
    h = h ^ s_hi
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m32
    h = h ^ (h >> np.uint64(16))
    if second:
        h = ((h ^ np.uint64(0x68E31DA4)) * np.uint64(0x2C1B3C6D)) & m32
        h = h ^ (h >> np.uint64(15))
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    ik = np.float32(1.0) / (np.float32(1.0) - p32)
    keep = np.where(u >= p32, ik, np.float32(0.0)).astype(np.float32)
    return torch.from_numpy(keep).reshape(M, D)


def _lora_ik(p) -> float:
    """1 / (1 - p) of the fp32 p, in double: what the kernels' fp32 quotient approximates."""
    return 1.0 / (1.0 - f32_value(p))


def lora_groups(D: int, R2: int) -> int:
    """Border groups mh_lora_down fills: 64 / R2, halved until every group's range of D is whole 32-element k-steps."""
    G = LORA_BORDER // R2
    while G > 1 and D % (32 * G):
        G >>= 1
    return G


def lora_rows(M: int, C: int, seed: int, scale: float = 1.0) -> torch.Tensor:
    """fp32 [M, C] token rows, by row index mod 4: N(0,1); 1e-3 N(0,1); 1e2 N(0,1); all zeros (times scale)."""
    x = rnd(M, C, seed=seed) * scale
    k = torch.arange(M) % 4
    x[k == 1] *= 1e-3
    x[k == 2] *= 1e2
    x[k == 3] = 0.0
    return x


def lora_adaptor(R2: int, D: int, seed: int) -> torch.Tensor:
    """fp32 A [R2, D] ~ 0.05 N(0,1) with one all-zero row (the last q row) and one row of 1.0 (the first v row)."""
    A = rnd(R2, D, seed=seed) * 0.05
    A[R2 // 2 - 1] = 0.0
    A[R2 // 2] = 1.0
    return A


def lora_down_ref_bound(x, A, s, p, keep_q, keep_v, R2, G):
    """fp64 partial borders of mh_lora_down (module docstring): dict part [M, G R2], part_bound, total [M, R2], total_bound."""
    x64, a64 = x.double(), A.to(torch.bfloat16).double()
    M, D = x64.shape
    r = R2 // 2
    ik = _lora_ik(p) if f32_value(p) > 0 else 1.0
    s = f32_value(s)
    xq, xv = x64 * (keep_q > 0), x64 * (keep_v > 0)
    w = D // G
    parts, bounds = [], []
    for g in range(G):
        c = slice(g * w, (g + 1) * w)
        sq, sv = xq[:, c] @ a64[:r, c].T, xv[:, c] @ a64[r:, c].T
        mq, mv = xq[:, c].abs() @ a64[:r, c].abs().T, xv[:, c].abs() @ a64[r:, c].abs().T
        ref = s * ik * torch.cat([sq, sv], 1)
        e = abs(s) * ik * g_acc(w, LORA_DOWN_WAVES) * torch.cat([mq, mv], 1) + (C_FN + 3) * U32 * ref.abs()
        parts.append(ref)
        bounds.append(bf16_out(ref, e))
    part, part_bound = torch.cat(parts, 1), torch.cat(bounds, 1)
    return dict(part=part, part_bound=part_bound, total=part.reshape(M, G, R2).sum(1), total_bound=part_bound.reshape(M, G, R2).sum(1))


def lora_dx_ref_bound(base, g, A, s, p, keep_q, keep_v):
    """fp64 (ref, bound) of mh_lora_dx: base [M, D], the border gradient g [M, R2], A [R2, D] fp32 (module docstring)."""
    b64, g64, a64 = base.double(), g.double(), A.to(torch.bfloat16).double()
    r = A.shape[0] // 2
    drop = f32_value(p) > 0
    ik = _lora_ik(p) if drop else 1.0
    s = f32_value(s)
    kq, kv = (keep_q > 0) * ik, (keep_v > 0) * ik
    tq, tv = g64[:, :r] @ a64[:r], g64[:, r:] @ a64[r:]
    mag = abs(s) * (kq * (g64[:, :r].abs() @ a64[:r].abs()) + kv * (g64[:, r:].abs() @ a64[r:].abs()))
    ref = b64 + s * (kq * tq + kv * tv)
    e = ((r + 3) + ((C_FN + 1) if drop else 0)) * U32 * mag + U32 * ref.abs()
    return ref, e


def lora_wgrad_ref_bound(x, keep_q, keep_v, sg_in, border, dq, dv, s, R2, mfma):
    """fp64 weight gradients of mh_lora_wgrad from what the kernel reads (module docstring): dict dA [R2, D], dBq, dBv [D, r] and
    *_bound."""
    x64, q64, v64 = x.double(), dq.double(), dv.double()
    M, D = x64.shape
    r = R2 // 2
    s = f32_value(s)
    sg = s * sg_in.double()
    grp = border.double().reshape(M, LORA_BORDER // R2, R2)
    st, e_st = grp.sum(1), 3 * U32 * grp.abs().sum(1)
    xq, xv = x64 * keep_q.double(), x64 * keep_v.double()          # the masks carry the fp32 quotient the kernels form too
    dA = torch.cat([sg[:, :r].T @ xq, sg[:, r:].T @ xv], 0)
    mA = torch.cat([sg[:, :r].abs().T @ xq.abs(), sg[:, r:].abs().T @ xv.abs()], 0)
    dBq, dBv = q64.T @ st[:, :r], v64.T @ st[:, r:]
    mBq, mBv = q64.abs().T @ st[:, :r].abs(), v64.abs().T @ st[:, r:].abs()
    if mfma:
        n = U16 * U16 + (4 * -(-(-(-M // LORA_WG_MFMA_CHUNKS)) // 32) + LORA_WG_MFMA_CHUNKS + C_FN + 4) * U32
    else:
        n = (-(-M // LORA_WG_CHUNKS) + LORA_WG_CHUNKS + 4) * U32
    return dict(dA=dA, dA_bound=n * mA, dBq=dBq, dBq_bound=n * mBq + q64.abs().T @ e_st[:, :r],
                dBv=dBv, dBv_bound=n * mBv + v64.abs().T @ e_st[:, r:])


def lora_refresh_check(ext, extT, Bq, Bv, W, D, r, what="lora_refresh"):
    """ext [>= 3W, >= D + 64] and extT [>= D + 64, >= 3W] (or None) started poisoned: every group of the border holds
    [bf16(B_q) | bf16(B_v)] -- B_q in the q rows (0..W), B_v in the v rows (2W..3W) -- and everything else is untouched: the k
    rows, the q rows' v columns and the v rows' q columns, the first D columns, the pad rows and columns."""
    q, v = Bq.to(torch.bfloat16), Bv.to(torch.bfloat16)
    own = torch.zeros(ext.shape, dtype=torch.bool, device=ext.device)
    ownT = None if extT is None else torch.zeros(extT.shape, dtype=torch.bool, device=extT.device)
    for g in range(LORA_BORDER // (2 * r)):
        c = D + g * 2 * r
        assert torch.equal(ext[:W, c:c + r], q), f"{what}: W_ext group {g} q"
        assert torch.equal(ext[2 * W:3 * W, c + r:c + 2 * r], v), f"{what}: W_ext group {g} v"
        own[:W, c:c + r] = True
        own[2 * W:3 * W, c + r:c + 2 * r] = True
        if extT is not None:
            assert torch.equal(extT[c:c + r, :W], q.T), f"{what}: W_ext^T group {g} q"
            assert torch.equal(extT[c + r:c + 2 * r, 2 * W:3 * W], v.T), f"{what}: W_ext^T group {g} v"
            ownT[c:c + r, :W] = True
            ownT[c + r:c + 2 * r, 2 * W:3 * W] = True
    assert bool(untouched(ext)[~own].all()), f"{what}: W_ext written outside the border's own cells"
    if extT is not None:
        assert bool(untouched(extT)[~ownT].all()), f"{what}: W_ext^T written outside the border's own cells"
