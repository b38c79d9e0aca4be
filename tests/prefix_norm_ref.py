"""Float64 restatement of the causal (prefix) energy normalisation (contract item 4) for the tests - oracle/ holds the
reference's utterance-level form only.  Differentiable torch; everything else of the G-step comes from oracle.nets as it is.

    P[t,c] = clean[t,c] ** inv_p;  S1[t] = cumsum_t sum_c P;  S2[t] = cumsum_t sum_c mask P
    ratio[t] = S1[t] / S2[t] where S2[t] > 0, else 1;  alpha2 = mask ratio;  enh = clean mask^p ratio^p
"""
import torch

from oracle.nets import d_inputs, discriminator_forward, generator_forward  # noqa: F401  (re-exported: the tests take them from here)


def prefix_sums(mask, clean_band, inv_p=6):
    """-> S1, S2 [B, T] in the dtype of the inputs (float64 in: the reference)."""
    P = torch.pow(clean_band.detach(), inv_p)
    return torch.cumsum(P.sum(dim=2), dim=1), torch.cumsum((mask * P).sum(dim=2), dim=1)


def prefix_ratio(mask, clean_band, inv_p=6):
    s1, s2 = prefix_sums(mask, clean_band, inv_p)
    ok = s2 > 0
    return torch.where(ok, s1 / torch.where(ok, s2, torch.ones_like(s2)), torch.ones_like(s2)), s1, s2


def prefix_energy_norm(mask, clean_band, p_power=1 / 6, inv_p=6):
    """-> (enh [B,T,64], ratio [B,T]) - the prefix counterpart of oracle.nets.energy_norm."""
    ratio, _, _ = prefix_ratio(mask, clean_band, inv_p)
    enh = clean_band * torch.pow(mask, p_power) * torch.pow(ratio, p_power).unsqueeze(2)
    return enh, ratio


def prefix_alpha2(mask, clean_band, inv_p=6):
    return mask * prefix_ratio(mask, clean_band, inv_p)[0].unsqueeze(2)


def prefix_dmask_closed_form(mask, clean_band, dE, p_power=1 / 6, inv_p=6):
    """The closed form the backward kernel implements, in the dtype of the inputs:
    dmask = dE clean p mask^(p-1) bp - K clean^inv_p,  bp = ratio^p,  K[t] = sum_{t'' >= t} (sum_c dE clean mask^p)[t''] p bp[t''] / S2[t'']."""
    ratio, _, s2 = prefix_ratio(mask, clean_band, inv_p)
    bp = torch.pow(ratio, p_power)
    R = (dE * clean_band * torch.pow(mask, p_power)).sum(dim=2)
    ok = s2 > 0
    w = torch.where(ok, R * p_power * bp / torch.where(ok, s2, torch.ones_like(s2)), torch.zeros_like(s2))
    K = torch.flip(torch.cumsum(torch.flip(w, dims=[1]), dim=1), dims=[1])
    return dE * clean_band * p_power * torch.pow(mask, p_power - 1) * bp.unsqueeze(2) - K.unsqueeze(2) * torch.pow(clean_band, inv_p)
