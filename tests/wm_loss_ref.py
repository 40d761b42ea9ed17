"""float64 references of the world-model loss stage (dreamer_amd/csrc/wm.hip) and of the reverse scan's row kernels
(ops.hip), one function per op of the dr_internal_wm_loss_run test hook, written from the formulas:

  masked losses, KL, free bits       WorldModel.py:125-138, 170-189
  two-hot reward target              DreamerUtils.to_twohot (primitives_ref.twohot_parts)
  continue loss                      binary_cross_entropy_with_logits
  straight-through sampler           VariationalAutoEncoder.py:92-98 (z = onehot + p - p.detach(), p = 0.99 softmax + 0.01 / C)
  LayerNorm(eps = 1e-5) + SiLU, gru_cell

Every function takes the float32 values the kernel reads and continues in float64.  The gradients of the backward
kernels come from float64 autograd of the forward restatement.  The free-bit factor d max(1, k) / dk is 1, 1/2, 0 for
k >, ==, < 1: torch's gradient of max at a tie, the convention k_wm_final documents.

`mut` names one deliberate break of a reference (MUTATIONS); tests/test_wm_loss_host.py checks that the inputs of
tests/test_gpu_wm_loss.py tell each of them from the reference by at least 100 tolerances.

tests/test_wm_loss_host.py pins these against oracle.dreamer_oracle on the CPU."""
import torch
import torch.nn.functional as F

import primitives_ref as PR

U = PR.U
F64 = torch.float64
f64 = PR.f64

# op codes of dr_internal_wm_loss_run (wm.hip WL_*)
(GATHER, PREP, KL_FWD, HEADS, STATS, FINAL, KL_BWD, STE_BWD_ADD, VEC_MSE, WINDOW_SCORES, GRU_BWD, LN_SILU_BWD,
 SOFTMAX_STE_BWD, COLSUM_MULTI) = range(14)
OP_NAMES = ["gather", "prep", "kl_fwd", "heads", "stats", "final", "kl_bwd", "ste_bwd_add", "vec_mse", "window_scores",
            "gru_bwd", "ln_silu_bwd", "softmax_ste_bwd", "colsum_multi"]

# mutation -> the op whose reference it breaks
MUTATIONS = {
    "wk_tie_is_1": "final",            # wk 0.5 -> 1 at KL == 1
    "kl_mean_over_mask": "final",      # KL mean over mask.sum() where it should be over rows
    "final_no_1e5": "final",           # 1e-5 dropped from the prediction loss's denominator
    "no_mask_in_cd_cr": "kl_bwd",      # mask dropped from cd / cr
    "no_klg_in_g_post": "kl_bwd",      # - klg dropped from g_post
    "coef_no_1e5": "prep",             # 1e-5 dropped from coef_row's denominator
    "coef_obs_no_2": "prep",           # coef_obs without its 2
    "searchsorted_left": "heads",      # searchsorted with right=False
    "no_nb2_clamp": "heads",           # the nb - 2 clamp missing
    "no_1e8": "heads",                 # 1e-8 dropped from the two-hot weight
    "ste_no_099": "ste_bwd_add",       # the 0.99 of the straight-through gradient missing
    "softmax_ste_no_099": "softmax_ste_bwd",
    "ln_var_km1": "ln_silu_bwd",       # LayerNorm variance over K - 1
    "gru_swap_ghn_gr": "gru_bwd",      # g_hn and g_r swapped
    "gru_ignore_accumulate": "gru_bwd",
}


# ----------------------------------------------------------------------------
# prep: window data, mask sum, row factors
# ----------------------------------------------------------------------------
def gather(actions, rewards, continues):
    """[B][T](*A) windows -> time-major rows m = t B + b (copies: exact)."""
    B, T = rewards.shape
    return dict(act_tm=f64(actions).transpose(0, 1).reshape(T * B, -1), rew_tm=f64(rewards).t().reshape(-1),
                cont_tm=f64(continues).t().reshape(-1))


def prep(cont, beta_pred, stats0=None, mut=None):
    """stats[0] = mask.sum() (or the all-reduced value a data-parallel caller wrote over it), scal[0] = it + 1e-5,
    coef_row = beta_pred mask / scal[0], coef_obs = 2 coef_row (the squared error's derivative)."""
    m = f64(cont)
    s0 = m.sum() if stats0 is None else f64(torch.tensor(stats0, dtype=torch.float32))
    denom = s0 + (0.0 if mut == "coef_no_1e5" else 1e-5)
    coef = float(torch.tensor(beta_pred, dtype=torch.float32)) * m / denom
    return dict(stats0=s0.reshape(1), scal0=denom.reshape(1), coef_row=coef,
                coef_obs=(1.0 if mut == "coef_obs_no_2" else 2.0) * coef)


# ----------------------------------------------------------------------------
# KL(post || prior) per latent group (WorldModel.py:175-183)
# ----------------------------------------------------------------------------
def cat_kl(post, prior):
    lp, lq = torch.log_softmax(post, -1), torch.log_softmax(prior, -1)
    return (lp.exp() * (lp - lq)).sum(-1)


def kl_fwd(prior, post):
    """prior, post: [M1, R, C] logits -> kl_grp [M1, R]."""
    return dict(kl_grp=cat_kl(f64(post), f64(prior)))


def kl_bwd(prior, post, cont, scal, mut=None):
    """Gradients of sum_rows mask (scal[1] KL(sg(post) || prior) + scal[2] KL(post || sg(prior))) by autograd."""
    q = f64(prior).clone().requires_grad_(True)
    p = f64(post).clone().requires_grad_(True)
    m = torch.ones_like(f64(cont)) if mut == "no_mask_in_cd_cr" else f64(cont)
    cd, cr = float(scal[1]) * m, float(scal[2]) * m
    loss = (cd * cat_kl(p.detach(), q).sum(-1)).sum() + (cr * cat_kl(p, q.detach()).sum(-1)).sum()
    g_prior, g_post = torch.autograd.grad(loss, [q, p])
    if mut == "no_klg_in_g_post":
        lp, lq = torch.log_softmax(p.detach(), -1), torch.log_softmax(q.detach(), -1)
        g_post = cr.reshape(-1, 1, 1) * lp.exp() * (lp - lq)
    return dict(g_prior=g_prior, g_post=g_post)


# ----------------------------------------------------------------------------
# reward two-hot log-likelihood and continue BCE per row (WorldModel.py:125-138)
# ----------------------------------------------------------------------------
def twohot_parts(v, buckets, mut=None):
    if mut is None:
        return PR.twohot_parts(v, buckets)
    v, b = f64(v), f64(buckets)
    nb = b.numel()
    vc = torch.clamp(v, min=float(b.min()), max=float(b.max()))
    lo = torch.searchsorted(b, vc.contiguous(), right=mut != "searchsorted_left") - 1
    lo = torch.clamp(lo, min=0, max=nb - 1 if mut == "no_nb2_clamp" else nb - 2)
    hi = torch.clamp(lo + 1, max=nb - 1)
    w = (vc - b[lo]) / (b[hi] - b[lo] + (0.0 if mut == "no_1e8" else 1e-8))
    return lo, w


def heads(rlog, clog, rew, cont, buckets, coef_row, mut=None):
    """rew_row = sum twohot(rew) log_softmax(rlog), cont_row = BCE-with-logits(clog, cont); g_rew, g_cont: autograd
    gradients of sum coef_row (-rew_row + cont_row) (both enter loss_pred with that sign, WorldModel.py:186)."""
    x = f64(rlog).clone().requires_grad_(True)
    xc = f64(clog).clone().requires_grad_(True)
    nb = x.shape[-1]
    lo, w = twohot_parts(rew, buckets, mut)
    hi = torch.clamp(lo + 1, max=nb - 1)
    ls = torch.log_softmax(x, -1)
    rew_row = (1.0 - w) * ls.gather(-1, lo.unsqueeze(-1)).squeeze(-1) + w * ls.gather(-1, hi.unsqueeze(-1)).squeeze(-1)
    cont_row = F.binary_cross_entropy_with_logits(xc, f64(cont), reduction="none")
    c = f64(coef_row)
    g_rew, g_cont = torch.autograd.grad((c * (cont_row - rew_row)).sum(), [x, xc])
    return dict(rew_row=rew_row.detach(), cont_row=cont_row.detach(), g_rew=g_rew, g_cont=g_cont)


# ----------------------------------------------------------------------------
# sums and the losses (WorldModel.py:170-189)
# ----------------------------------------------------------------------------
def stats_terms(obs_part, rew_row, cont_row, kl_grp, cont):
    """The masked per-row terms whose sums are stats[1..4]: [4, M1]."""
    m = f64(cont)
    return torch.stack([f64(obs_part).sum(-1) * m, f64(rew_row) * m, f64(cont_row) * m, f64(kl_grp).sum(-1) * m])


def stats(obs_part, rew_row, cont_row, kl_grp, cont):
    return dict(stats=stats_terms(obs_part, rew_row, cont_row, kl_grp, cont).sum(-1))


def final(stats5, rows, betas, mut=None):
    """stats5: mask.sum() and the four masked sums; rows = B_global (T - 1), torch.mean's count.  Returns losses
    (total, pred, kl, kl), scal[1], scal[2] (the KL gradients' factors) and skip."""
    s = f64(stats5)
    bp, bd, br = (float(torch.tensor(b, dtype=torch.float32)) for b in betas)
    pred = (s[1] - s[2] + s[3]) / (s[0] + (0.0 if mut == "final_no_1e5" else 1e-5))
    n = s[0] if mut == "kl_mean_over_mask" else float(rows)
    kl = (s[4] / n).clone().requires_grad_(True)
    one = torch.ones((), dtype=F64)
    total = bp * pred + bd * torch.max(one, kl) + br * torch.max(one, kl)
    wk = torch.autograd.grad(torch.max(one, kl), kl)[0]  # 1, 1/2, 0
    if mut == "wk_tie_is_1" and float(kl.detach()) == 1.0:
        wk = one
    kl = kl.detach()
    losses = torch.stack([total.detach(), pred, kl, kl])
    return dict(losses=losses, scal1=(bd * wk / n).reshape(1), scal2=(br * wk / n).reshape(1),
                skip=0 if bool(torch.isfinite(total)) else 1)


def window_scores(obs_part, rew_row, cont_row, kl_grp, cont, B, betas):
    """Per-window loss, rows m = t B + b: beta_pred sum_t mask (obs - rew + cont) / (sum_t mask + 1e-5) +
    (beta_dyn + beta_rep) mean_t (mask KL), no free-bit clamp."""
    t = stats_terms(obs_part, rew_row, cont_row, kl_grp, cont).reshape(4, -1, B)
    m = f64(cont).reshape(-1, B)
    bp, bd, br = (float(torch.tensor(b, dtype=torch.float32)) for b in betas)
    pred = (t[0] - t[1] + t[2]).sum(0) / (m.sum(0) + 1e-5)
    return dict(scores=bp * pred + (bd + br) * t[3].mean(0))


def vec_mse(mu, x, coef):
    """part = sum (mu - x)^2 per row; g = d/dmu of sum_rows coef / 2 part (coef carries the 2)."""
    m = f64(mu).clone().requires_grad_(True)
    part = ((m - f64(x)) ** 2).sum(-1)
    g, = torch.autograd.grad((0.5 * f64(coef) * part).sum(), m)
    return dict(part=part.detach(), g=g)


# ----------------------------------------------------------------------------
# straight-through sampler backward (VariationalAutoEncoder.py:92-98)
# ----------------------------------------------------------------------------
def ste_logits(soft):
    """Logits whose softmax is `soft` (the kernel reads the saved softmax, not the logits)."""
    return torch.log(f64(soft))


def ste_bwd(gz, soft, extra=None, mut=None):
    """dL/dlogits of z = onehot + p - p.detach(), p = 0.99 softmax(logits) + 0.01 / C, given gz = dL/dz, by autograd
    at logits = log(soft); (+ extra: the KL-rep gradient of the same logits)."""
    x = ste_logits(soft).clone().requires_grad_(True)
    C = x.shape[-1]
    s = torch.softmax(x, -1)
    p = (1.0 if mut in ("ste_no_099", "softmax_ste_no_099") else 0.99) * s + 0.01 / C
    z = p - p.detach()
    gl, = torch.autograd.grad((z * f64(gz)).sum(), x)
    return dict(gl=gl if extra is None else gl + f64(extra))


# ----------------------------------------------------------------------------
# GRU gates backward (gru_cell: r = sig(ir + hr), u = sig(iz + hz), n = tanh(in + r hn), h' = (h - n) u + n)
# ----------------------------------------------------------------------------
def gru_bwd(g_hp, h, sr, su, sn, sghn, gh_prev, accumulate, mut=None):
    """The kernel reads the saved gates; the restatement is evaluated at the pre-activations that give exactly those
    gates in float64 (logit, atanh; a gate of exactly 0 / 1 / +-1 sits at an infinite pre-activation, where sigmoid'
    and tanh' are 0).  g_gi = dL/d(ir, iz, in), g_gh = dL/d(hr, hz, hn), gh_out = (gh_prev +) dL/dh's direct path."""
    r0, u0, n0, hn0 = f64(sr), f64(su), f64(sn), f64(sghn)
    hv = torch.zeros_like(r0) if h is None else f64(h)
    gi = torch.cat([torch.logit(r0), torch.logit(u0), torch.atanh(n0) - r0 * hn0], -1).requires_grad_(True)
    gh = torch.cat([torch.zeros_like(r0), torch.zeros_like(r0), hn0], -1).requires_grad_(True)
    hl = hv.clone().requires_grad_(True)
    i_r, i_z, i_n = gi.chunk(3, -1)
    h_r, h_z, h_n = gh.chunk(3, -1)
    r, u = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    hp = (hl - n) * u + n
    g_gi, g_gh, g_h = torch.autograd.grad((hp * f64(g_hp)).sum(), [gi, gh, hl])
    if mut == "gru_swap_ghn_gr":
        Hd = r0.shape[-1]
        g_pn = g_gi[:, 2 * Hd:]
        g_gh = torch.cat([g_gh[:, :2 * Hd], g_pn * hn0], -1)
    if accumulate and mut != "gru_ignore_accumulate":
        g_h = g_h + f64(gh_prev)
    return dict(g_gi=g_gi, g_gh=g_gh, gh_out=g_h)


# ----------------------------------------------------------------------------
# LayerNorm(eps = 1e-5) + SiLU backward
# ----------------------------------------------------------------------------
def layer_norm(x, gamma, beta, mut=None):
    K = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / (K - 1 if mut == "ln_var_km1" and K > 1 else K)
    xhat = d / torch.sqrt(var + 1e-5)
    return xhat, xhat * gamma + beta


def ln_silu_bwd(gx, pre, gamma, beta, mut=None):
    """gx = dL/d SiLU(LN(pre)).  g_pre = dL/dpre and gy = dL/d(LN output) by autograd; xhat the normalised row."""
    p = f64(pre).clone().requires_grad_(True)
    xhat, y = layer_norm(p, f64(gamma), f64(beta), mut)
    y.retain_grad()
    (F.silu(y) * f64(gx)).sum().backward()
    return dict(g_pre=p.grad, gy=y.grad, xhat=xhat.detach())


def bf16_rne(x32):
    """The bf16 round-to-nearest-even of float32 values, as uint16 bit patterns (in an int32 tensor)."""
    b = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return (r & 0xFFFF).to(torch.int32)


def colsum(X, Y=None, prev=None):
    t = f64(X) if Y is None else f64(X) * f64(Y)
    s = t.sum(0)
    return dict(out=s if prev is None else s + f64(prev), abs=t.abs().sum(0))
