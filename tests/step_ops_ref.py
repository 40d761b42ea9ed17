"""float64 references of the recurrent step's and the actor head's row kernels (dreamer_amd/csrc/gru.hip and the first
half of ops.hip), one function per op of the dr_internal_step_run test hook, written from the definitions:

  GRU step                 SequenceModel.py:19-24 -> torch gru_cell: gi = W_ih cat(flatten(z), a) + b_ih, gh = W_hh h + b_hh,
                           r = sig(gi_r + gh_r), u = sig(gi_u + gh_u), n = tanh(gi_n + r gh_n), h' = (h - n) u + n
  actor head               Agent.py:191-210: ls = clamp(ls_raw, -5, 2), sigma = softplus(ls) + 1e-3, a = tanh(mu + eps sigma)
  straight-through sampler VAE.py:88-98, DynamicsPredictors.py:33-39: p = softmax, pu = 0.99 p + 0.01 / C,
                           winner = argmax(pu / sum(pu) / q), z = onehot + pu - pu.detach()
  continue probability     DynamicsPredictors.py:95-105: sigmoid

Every function takes the float32 values the kernel reads and continues in float64.  The GRU's input product is DENSE
on the whole latent row: gathered one-hot groups, straight-through values off 1 and groups with several non-zero
classes all go through the one formula, and the kernels' gather (idx, zval, the dense marker) is what is under test.

The actor head's backward is a closed form on the kernel's own inputs (the saved float32 a, eps, ls_raw):
g_p = g_a (1 - a^2) with a as given -- float64 autograd from mu would use 1 - tanh^2, which differs from the kernel's
contract by the rounding of a, unbounded in relative terms near saturation; g_mu = g_mu_l + g_p; g_sig = g_sig_l +
g_p eps; g_ls = g_sig sigmoid(ls) for -5 <= ls <= 2 (closed at both ends, like torch.clamp's gradient), else 0;
gx = g_heads wt^T.

`mut` names one deliberate break of a reference (MUTATIONS); tests/test_step_ops_host.py checks that the inputs of
tests/test_gpu_step_ops.py tell each from the reference by at least 100 tolerances, and pins the references against
oracle.dreamer_oracle on the CPU."""
import torch

import primitives_ref as PR
from wm_loss_ref import bf16_rne

U = PR.U
F32 = torch.float32
F64 = torch.float64
f64 = PR.f64

# op codes of dr_internal_step_run (step_hook.hip SO_*)
(GRU, ONEHOT_INDEX, ZGATHER_ADD, GRU_FWD, SAMPLE, ACTOR_HEAD, ACTOR_HEAD_BWD_X, SIGMOID, MEAN, TRANSPOSE,
 TRANSPOSE_MULTI, COPY2D, COPY2D_MULTI, FILL, VEC_GATHER) = range(15)
OP_NAMES = ["gru", "onehot_index", "zgather_add", "gru_fwd", "sample", "actor_head", "actor_head_bwd_x", "sigmoid",
            "mean", "transpose", "transpose_multi", "copy2d", "copy2d_multi", "fill", "vec_gather"]

# mutation -> the op whose reference it breaks
MUTATIONS = {
    "gru_swap_r_u": "gru",              # r and u swapped
    "gru_r_on_whole_n": "gru",          # r applied to gi_n + gh_n
    "gru_blend_reversed": "gru",        # h' = (n - h) u + h
    "gru_no_bhh_n": "gru",              # b_hh dropped on the n gate
    "gru_drop_last_action": "gru",
    "gru_drop_last_group": "gru",
    "gru_zval_as_1": "gru",             # the straight-through value read as 1
    "gru_dense_first_only": "gru",      # a dense group read as its first non-zero class only
    "gru_idx_off_by_one": "gru",
    "gru_last_row_row0_idx": "gru",     # the last row takes row 0's indices (a tile-edge slip)
    "gru_h_null_as_ones": "gru",
    "gru_bf16_truncate": "gru",         # hout16 truncated where it should round to nearest even
    "zg_drop_last_group": "zgather_add",
    "zg_zval_as_1": "zgather_add",
    "zg_dense_first_only": "zgather_add",
    "zg_idx_off_by_one": "zgather_add",
    "zg_last_row_row0_idx": "zgather_add",
    "bwd_clamp_open": "actor_head_bwd_x",       # no gradient at exactly -5 and 2
    "bwd_softplus_slope_1": "actor_head_bwd_x",
    "bwd_eps_wrong_row": "actor_head_bwd_x",    # g_sig takes eps of the next row
    "head_sigma_no_1e3": "actor_head",
    "sample_no_unimix": "sample",
    "sample_q_step0": "sample",
    "mean_n_1024": "mean",              # mean over n rounded up to a multiple of 1024
    "transpose_ignores_ldo": "transpose_multi",
}


# ----------------------------------------------------------------------------
# the one-hot index (k_onehot_index) and the mutants that act on the latent row
# ----------------------------------------------------------------------------
def onehot_index(z):
    """z [M][R][C] -> idx [M][R] (int64), zval [M][R] (float32, the value itself): no non-zero class (0, 0), one
    (k, v), two or more (-1, 0).  -0.0 is zero; NaN is not."""
    nz = z != 0
    cnt = nz.sum(-1)
    first = torch.argmax(nz.to(torch.int8), -1)
    v = torch.gather(z, -1, first.unsqueeze(-1)).squeeze(-1)
    idx = torch.where(cnt > 1, torch.full_like(first, -1), torch.where(cnt == 1, first, torch.zeros_like(first)))
    zval = torch.where(cnt == 1, v, torch.zeros_like(v))
    return idx, zval


def mutate_latent(z, mut):
    """The latent rows a kernel with the named slip would effectively use."""
    z = z.clone()
    M, R, C = z.shape
    idx, zval = onehot_index(z)
    one = idx >= 0  # gathered groups
    if mut == "drop_last_group":
        z[:, R - 1] = 0
    elif mut == "zval_as_1":
        z = torch.where(one.unsqueeze(-1) & (z != 0), torch.ones_like(z), z)
    elif mut == "dense_first_only":
        nz = z != 0
        first = torch.argmax(nz.to(torch.int8), -1, keepdim=True)
        keep = torch.zeros_like(nz).scatter_(-1, first, True)
        z = torch.where((~one).unsqueeze(-1) & ~keep, torch.zeros_like(z), z)
    elif mut == "idx_off_by_one":
        moved = torch.zeros_like(z).scatter_(-1, ((idx + 1) % C).clamp(min=0).unsqueeze(-1), zval.unsqueeze(-1))
        z = torch.where(one.unsqueeze(-1), moved, z)
    elif mut == "last_row_row0_idx":
        use = one[M - 1] & one[0]
        moved = torch.zeros_like(z[0]).scatter_(-1, idx[0].clamp(min=0).unsqueeze(-1), zval[M - 1].unsqueeze(-1))
        z[M - 1] = torch.where(use.unsqueeze(-1), moved, z[M - 1])
    return z


# ----------------------------------------------------------------------------
# GRU
# ----------------------------------------------------------------------------
def gru_gates(gi, gh, h, mut=None, gi_abs=None, gh_abs=None):
    """The gate block on gi, gh [B][3 Hd] (biases included) in float64; h None = zeros."""
    Hd = gi.shape[1] // 3
    i_r, i_u, i_n = gi[:, :Hd], gi[:, Hd:2 * Hd], gi[:, 2 * Hd:]
    h_r, h_u, h_n = gh[:, :Hd], gh[:, Hd:2 * Hd], gh[:, 2 * Hd:]
    r, u = torch.sigmoid(i_r + h_r), torch.sigmoid(i_u + h_u)
    if mut == "gru_swap_r_u":
        r, u = u, r
    n = torch.tanh((i_n + h_n) * r if mut == "gru_r_on_whole_n" else i_n + h_n * r)
    hv = torch.zeros_like(n) if h is None else h
    if mut == "gru_h_null_as_ones" and h is None:
        hv = torch.ones_like(n)
    hp = (n - hv) * u + hv if mut == "gru_blend_reversed" else (hv - n) * u + n
    out = dict(hout=hp, sr=r, su=u, sn=n, sghn=h_n)
    if gi_abs is not None:  # sum |terms| of the three pre-activations, the scale of their rounding
        s = gi_abs + gh_abs
        out.update(abs_r=s[:, :Hd], abs_u=s[:, Hd:2 * Hd], abs_n=s[:, 2 * Hd:], abs_ghn=gh_abs[:, 2 * Hd:], habs=hv.abs())
    return out


def gru(z, a, h, wt, b_ih, w_hh, b_hh, mut=None):
    """z [B][R][C] the latent rows, a [B][A], h [B][Hd] or None, wt = W_ih^T [R C + A][3 Hd], w_hh [3 Hd][Hd]."""
    B, R, C = z.shape
    Hd = w_hh.shape[1]
    if mut and mut.startswith("gru_") and mut[4:] in ("drop_last_group", "zval_as_1", "dense_first_only",
                                                     "idx_off_by_one", "last_row_row0_idx"):
        z = mutate_latent(z, mut[4:])
    a = a.clone()
    if mut == "gru_drop_last_action" and a.shape[1]:
        a[:, -1] = 0
    x = torch.cat([f64(z).reshape(B, R * C), f64(a)], 1)
    # NaN-free padding of a dense product: 0 * w is 0 here (the operands are finite wherever the case is)
    W = f64(wt)
    gi = x @ W + f64(b_ih)
    gi_abs = x.abs() @ W.abs() + f64(b_ih).abs()
    bh = f64(b_hh).clone()
    if mut == "gru_no_bhh_n":
        bh[2 * Hd:] = 0
    if h is None:
        gh = bh.expand(B, 3 * Hd).clone()
        gh_abs = bh.abs().expand(B, 3 * Hd).clone()
    else:
        gh = f64(h) @ f64(w_hh).t() + bh
        gh_abs = f64(h).abs() @ f64(w_hh).abs().t() + bh.abs()
    out = gru_gates(gi, gh, None if h is None else f64(h), mut, gi_abs, gh_abs)
    out["gh"] = gh
    out["gh_abs"] = gh_abs
    return out


def bf16_bits(x32, mut=None):
    """hout16 of a float32 h': round to nearest even, as int32 holding the uint16 pattern."""
    if mut == "gru_bf16_truncate":
        return ((x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF) >> 16).to(torch.int32)
    return bf16_rne(x32)


# ----------------------------------------------------------------------------
# zgather_add
# ----------------------------------------------------------------------------
def zgather_add(z, wt, base, mut=None):
    """z [M][R][C], wt [R C][N], base [M][N] -> out, and sum |terms| of out - base."""
    if mut and mut.startswith("zg_"):
        z = mutate_latent(z, mut[3:])
    M = z.shape[0]
    x = f64(z).reshape(M, -1)
    return dict(out=f64(base) + x @ f64(wt), abs=x.abs() @ f64(wt).abs())


# ----------------------------------------------------------------------------
# sampler
# ----------------------------------------------------------------------------
def sample(logits, q, step=0, mut=None):
    """logits [M][R][C], q [steps][M R][C] -> p (softmax), score = pu / sum(pu) / q[step], win [M][R], and `margin`,
    the relative gap between the best and the second-best score (inf for C == 1)."""
    M, R, C = logits.shape
    p = torch.softmax(f64(logits), -1)
    pu = p if mut == "sample_no_unimix" else f64(torch.tensor(0.99, dtype=F32)) * p + f64(torch.tensor(0.01 * (1.0 / C), dtype=F32))
    ph = pu / pu.sum(-1, keepdim=True)
    score = ph / f64(q[0 if mut == "sample_q_step0" else step]).reshape(M, R, C)
    win = torch.argmax(score, -1)
    if C > 1:
        top = torch.topk(score, 2, -1).values
        margin = (top[..., 0] - top[..., 1]) / top[..., 0]
    else:
        margin = torch.full((M, R), float("inf"), dtype=F64)
    return dict(p=p, pu=pu, score=score, win=win, margin=margin)


def ste_value(soft32, C):
    """The straight-through value the sampler writes at the winner, (1 + pu) - pu in float32 on its own soft."""
    pu = torch.tensor(0.99, dtype=F32) * soft32 + torch.tensor(0.01 * (1.0 / C), dtype=F32)
    return (1.0 + pu) - pu


# ----------------------------------------------------------------------------
# actor head
# ----------------------------------------------------------------------------
E3 = float(torch.tensor(1e-3, dtype=F32))


def actor_head(mu_raw, ls_raw, eps, det, mut=None):
    mu, ls = f64(mu_raw), f64(ls_raw).clamp(-5.0, 2.0)
    sp = torch.nn.functional.softplus(ls)
    sigma = sp + (0.0 if mut == "head_sigma_no_1e3" else E3)
    pre = mu if det else mu + f64(eps) * sigma
    pre_abs = mu.abs() if det else mu.abs() + (f64(eps) * sigma).abs()
    return dict(a=torch.tanh(pre), mu=mu, sigma=sigma, pre_abs=pre_abs)


def actor_head_bwd_x(g_a, g_mu_l, g_sig_l, a, ls_raw, eps, wt, mut=None):
    """g_a, g_mu_l, g_sig_l [M][A] or None; a, ls_raw, eps [M][A]; wt [N][2 A] -> g_heads [M][2 A], gx [M][N] and the
    sizes of what they are made of."""
    ls = f64(ls_raw)
    zero = torch.zeros_like(ls)
    g_mu = zero.clone() if g_mu_l is None else f64(g_mu_l)
    g_sig = zero.clone() if g_sig_l is None else f64(g_sig_l)
    mu_abs, sig_abs = g_mu.abs(), g_sig.abs()
    if g_a is not None:
        e = f64(eps)
        if mut == "bwd_eps_wrong_row":
            e = torch.roll(e, -1, 0)
        g_p = f64(g_a) * (1.0 - f64(a) ** 2)
        g_mu = g_mu + g_p
        g_sig = g_sig + g_p * e
        mu_abs = mu_abs + f64(g_a).abs()
        sig_abs = sig_abs + (f64(g_a) * e).abs()
    inside = (ls > -5.0) & (ls < 2.0) if mut == "bwd_clamp_open" else (ls >= -5.0) & (ls <= 2.0)
    slope = torch.ones_like(ls) if mut == "bwd_softplus_slope_1" else torch.sigmoid(ls.clamp(-5.0, 2.0))
    g_ls = torch.where(inside, g_sig * slope, zero)
    g_heads = torch.cat([g_mu, g_ls], 1)
    W = f64(wt)
    return dict(g_heads=g_heads, heads_abs=torch.cat([mu_abs, torch.where(inside, sig_abs, zero)], 1),
                gx=g_heads @ W.t(), W_abs=W.abs())


# ----------------------------------------------------------------------------
# the small ones
# ----------------------------------------------------------------------------
def sigmoid(x):
    return torch.sigmoid(f64(x))


def mean(x, mut=None):
    n = x.numel()
    if mut == "mean_n_1024":
        n = -(-n // 1024) * 1024
    return dict(out=(f64(x).sum() / n).reshape(1), abs=(f64(x).abs().sum() / x.numel()).reshape(1))


def transpose(x):
    """out[c * ldo + r] = in[r * cols + c]: the [cols][ldo] buffer's written part, [cols][rows]."""
    return f64(x).t().contiguous()


def vec_gather(n, nb, D, ring=None, ring_cap=0, starts=None, obs=None, stride_b=0, stride_t=0, t0=0):
    """X[f][c] for frame f = t nb + b: ring[((starts[b] + t0 + t) % ring_cap) D + c] or obs[b stride_b + (t0 + t) stride_t + c]."""
    X = torch.empty(n, D, dtype=F64)
    for f in range(n):
        b, t = f % nb, f // nb + t0
        if ring is not None:
            s = int((int(starts[b]) + t) % ring_cap) * D
            X[f] = f64(ring.reshape(-1)[s:s + D])
        else:
            s = b * stride_b + t * stride_t
            X[f] = f64(obs.reshape(-1)[s:s + D])
    return X
