"""float64 restatements of the networks' glue kernels (disc.hip, gen.hip), shared by test_glue_exact_gpu.py (the references the kernels are
held to) and test_glue_refs_cpu.py (which holds these restatements to float64 autograd of oracle/nets.py).  Plain torch, any device; every
function computes in the dtype of its inputs, so the same closed form can be evaluated in float32 to measure what float32 arithmetic costs.
"""
import numpy as np
import torch

P32 = float(np.float32(1.0 / 6.0))          # the exponent every caller passes, as the kernels see it
INV_P = 6.0


def energy_inputs(B, T, seed, zero_tail=()):
    """band features as the feature kernels leave them (positive; the frames behind zero_tail[b] exact zeros), a mask in exp(3.2 tanh)'s
    range, a random d(din) [B][64][T][4]; numpy float32"""
    rs = np.random.RandomState(seed)
    clean = (0.1 + 0.4 * rs.rand(B, T, 64)).astype(np.float32)
    noise = (0.1 + 0.4 * rs.rand(B, T, 64)).astype(np.float32)
    mask = np.exp(3.2 * np.tanh(rs.randn(B, T, 64))).astype(np.float32)
    ddin = rs.randn(B, 64, T, 4).astype(np.float32)
    for b, n in enumerate(zero_tail):
        clean[b, n:] = 0
        noise[b, n:] = 0
    return clean, mask, noise, ddin


def energy_norm_sums(mask, clean, inv_p=INV_P):
    """S1 = sum clean^inv_p, S2 = sum mask clean^inv_p per utterance ([B]); mask, clean [B][T][64]"""
    cp = clean ** inv_p
    return cp.sum((1, 2)), (mask * cp).sum((1, 2))


def energy_norm_enh(mask, clean, p=P32, inv_p=INV_P):
    """train_nele.py:133-140: clean mask^p (S1 / S2)^p and beta2 = S1 / S2"""
    s1, s2 = energy_norm_sums(mask, clean, inv_p)
    beta2 = s1 / s2
    return clean * mask ** p * (beta2 ** p)[:, None, None], beta2


def energy_norm_dmask(mask, clean, dE, p=P32, inv_p=INV_P):
    """gradient of sum(dE * enh) with respect to the mask, clean^inv_p held constant (it is detached in the reference):
    dm = dE clean p mask^(p-1) bp - (sum dE clean mask^p) p bp / S2 clean^inv_p,  bp = (S1 / S2)^p;  dE [B][T][64]"""
    s1, s2 = energy_norm_sums(mask, clean, inv_p)
    bp = ((s1 / s2) ** p)[:, None, None]
    r = (dE * clean * mask ** p).sum((1, 2))[:, None, None]
    return dE * clean * p * mask ** (p - 1) * bp - r * p * bp / s2[:, None, None] * clean ** inv_p


def sn_grad(dW, W, u, v, sigma):
    """gradient through W / sigma with u, v constant and sigma = u . (W v): (dW - <dW, W / sigma> u v^T) / sigma; -> (value, the dot product,
    its magnitude sum)"""
    dot = (dW * W / sigma).sum()
    return (dW - dot * torch.outer(u, v)) / sigma, dot, (dW * W / sigma).abs().sum()


def spectral_norm_step(W, u):
    """one power iteration of torch.nn.utils.spectral_norm: v = normalize(W^T u), u = normalize(W v), sigma = u . (W v)"""
    a = W.t() @ u
    v = a / a.norm().clamp_min(1e-12)
    wv = W @ v
    u = wv / wv.norm().clamp_min(1e-12)
    return u, v, u @ (W @ v)


def head_forward(pooled, ws, bs, sg, slope=0.3):
    """model.py:124-132 on pooled [B][64]: Linear(W / sigma) + LeakyReLU twice, Linear + sigmoid; -> h1, h2, score"""
    x, outs = pooled, []
    for q in range(3):
        z = x @ (ws[q] / sg[q]).T + bs[q]
        x = torch.where(z > 0, z, slope * z) if q < 2 else torch.sigmoid(z)
        outs.append(x)
    return outs


def gap_backward(dpooled, act, wvalid, slope=0.3):
    """gradient of mean over (Hout, columns < wvalid[b]) of act [B][Hout][Wout][64] = LeakyReLU(z), with respect to z"""
    B, Hout, Wout, _ = act.shape
    out = torch.zeros_like(act)
    for b in range(B):
        wv = int(wvalid[b])
        out[b, :, :wv] = dpooled[b] / (Hout * wv) * torch.where(act[b, :, :wv] > 0, act.new_tensor(1.0), act.new_tensor(slope))
    return out


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    """torch.optim.Adam (no amsgrad, no weight decay), one step; -> p, m, v, and the terms the float32 error bound is made of"""
    m1, m2 = beta1 * m, (1 - beta1) * g
    v1, v2 = beta2 * v, (1 - beta2) * g * g
    mn, vn = m1 + m2, v1 + v2
    denom = vn.sqrt() / np.sqrt(1 - beta2 ** step) + eps
    step_size = lr / (1 - beta1 ** step)
    upd = step_size * mn / denom
    return p - upd, mn, vn, dict(m_mag=m1.abs() + m2.abs(), v_mag=v1 + v2, upd=upd, gain=step_size / denom)
