"""CPU: the float64 restatements the kernel tests compare against (tests/glue_refs.py, exact_rules._head_ref) agree with float64 autograd
of oracle/nets.py, and every shape of the integer rule keeps its sums below 2^24 (tests/f32_cases.py)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import f32_cases as cases  # noqa: E402
import glue_refs as ref  # noqa: E402
from oracle import nets  # noqa: E402


def _close(a, b, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * float(b.abs().max()), float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('B,T,tail', [(3, 57, ()), (2, 129, (129, 70)), (1, 1, ())])
def test_energy_norm_closed_form_is_the_autograd_of_the_oracle(B, T, tail):
    clean, mask, _, ddin = [torch.from_numpy(a).double() for a in ref.energy_inputs(B, T, 7 * B + T, tail)]
    dE = ddin[..., 0].permute(0, 2, 1)
    m = mask.clone().requires_grad_(True)
    enh, beta2 = nets.energy_norm(m, clean, ref.P32, 6)
    (enh * dE).sum().backward()
    e2, b2 = ref.energy_norm_enh(mask, clean)
    _close(e2, enh.detach())
    _close(b2, beta2.detach())
    _close(ref.energy_norm_dmask(mask, clean, dE), m.grad)
    if tail:
        assert float(m.grad[1, tail[1]:].abs().max()) == 0     # a zero frame's mask moves nothing


def test_spectral_norm_step_and_weight_gradient_are_the_oracles():
    g = torch.Generator().manual_seed(3)
    for N, K in ((3, 4), (16, 63), (64, 3888)):
        W = torch.randn((N, K), generator=g, dtype=torch.float64)
        u0 = torch.nn.functional.normalize(torch.randn(N, generator=g, dtype=torch.float64), dim=0)
        v0 = torch.nn.functional.normalize(torch.randn(K, generator=g, dtype=torch.float64), dim=0)
        G = torch.randn((N, K), generator=g, dtype=torch.float64)
        Wp = W.clone().requires_grad_(True)
        nb = {}
        wn = nets._sn_weight({'l.weight_orig': Wp, 'l.weight_u': u0, 'l.weight_v': v0}, 'l', True, nb)
        (wn * G).sum().backward()
        u, v, sigma = ref.spectral_norm_step(W, u0)
        _close(u, nb['l.weight_u'])
        _close(v, nb['l.weight_v'])
        _close(wn.detach(), W / sigma)
        val, _, _ = ref.sn_grad(G, W, u, v, sigma)
        _close(val, Wp.grad)


def test_head_restatements_are_the_autograd_of_the_oracle():
    from exact_rules import _head_ref
    g = torch.Generator().manual_seed(5)
    B, Hout, Wout, nout = 3, 5, 9, 3
    wvalid = [9, 4, 1]
    rn = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)  # noqa: E731
    sd = {}
    for name, (n, k) in (('fc1', (64, 64)), ('fc2', (16, 64)), ('fc3', (nout, 16))):
        sd[name + '.weight_orig'], sd[name + '.bias'] = rn(n, k) / np.sqrt(k), 0.1 * rn(n)
        sd[name + '.weight_u'] = torch.nn.functional.normalize(rn(n), dim=0)
        sd[name + '.weight_v'] = torch.nn.functional.normalize(rn(k), dim=0)
    z = rn(B, Hout, Wout, 64).requires_grad_(True)
    act = torch.nn.functional.leaky_relu(z, 0.3)
    pooled = torch.stack([act[b, :, :wvalid[b]].mean((0, 1)) for b in range(B)])       # model.py:123, every utterance over its own extent
    pooled.retain_grad()
    h, hs = pooled, []
    for q, name in enumerate(('fc1', 'fc2', 'fc3')):
        h = torch.nn.functional.linear(h, nets._sn_weight(sd, name, False, {}), sd[name + '.bias'])
        h = torch.nn.functional.leaky_relu(h, 0.3) if q < 2 else torch.sigmoid(h)
        hs.append(h)
    dscore = rn(B, nout)
    (h * dscore).sum().backward()
    ws = [sd[n + '.weight_orig'] for n in ('fc1', 'fc2', 'fc3')]
    bs = [sd[n + '.bias'] for n in ('fc1', 'fc2', 'fc3')]
    sg = [torch.dot(sd[n + '.weight_u'], sd[n + '.weight_orig'] @ sd[n + '.weight_v']).reshape(1) for n in ('fc1', 'fc2', 'fc3')]
    for got, (want, S), want2 in zip(hs, _head_ref(pooled.detach(), ws, bs, sg), ref.head_forward(pooled.detach(), ws, bs, sg)):
        _close(want, got.detach())
        _close(want2, got.detach())
        assert bool((S >= want.abs() - 1e-12).all())
    _close(ref.gap_backward(pooled.grad, act.detach(), wvalid), z.grad)


def test_adam_restatement_is_torch_adam():
    g = torch.Generator().manual_seed(9)
    p = torch.randn(300, generator=g, dtype=torch.float64)
    q = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in (1, 2, 3):
        grad = torch.randn(300, generator=g, dtype=torch.float64)
        q.grad = grad.clone()
        opt.step()
        p, m, v, _ = ref.adam_step(p, grad, m, v, 1e-3, 0.9, 0.999, 1e-8, step)
        _close(p, q.detach())


def test_every_integer_rule_shape_keeps_its_sums_below_2_to_24():
    bounds = cases.integer_rule_bounds()
    assert len(bounds) > 80
    for tag, b in bounds:
        assert b < cases.LIMIT, (tag, b)
    # the largest reduction of each kind, spelled out: K = 81 * 64 (D.layers.4's data gradient), M = 2 * 44 * 65 (its weight gradient at T = 85)
    assert dict(bounds)['span.D4.dgrad'] == 8 * 5184 and dict(bounds)['wgrad.D4.T85'] == 8 * 5720 + 8


def test_the_case_lists_reach_every_variant():
    """every TN x TM of conv_gemm_kernel, every NT of conv_span_kernel, the split counts of the weight gradient"""
    tn = lambda N: min((N + 15) // 16, 4)  # noqa: E731
    assert {(tn(N), tm) for N, M, tm in cases.gemm_tm_cases()} == {(a, b) for a in (1, 2, 3, 4) for b in (1, 2, 4)}
    for N, M, tm in cases.gemm_tm_cases():
        assert cases.gemm_tm(M, N) == tm and M % 64 != 0
    assert {c[5] for c in cases.gemm_cases()} >= {4, 8, 16, 20, 32, 48, 64, 80, 256}
    assert {(N + 15) // 16 for _, C, N, K in cases.SPAN_LAYERS} == {1, 2, 3, 4} and {N for _, C, N, K in cases.SPAN_LAYERS} == {4, 8, 16, 32, 48, 64}
    for W in cases.SPAN_WIDTHS:
        assert W >= 64 and ((cases.SPAN_B * cases.span_hout(W) * W) % 256 != 0 or W == 256)
