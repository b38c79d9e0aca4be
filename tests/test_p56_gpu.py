"""GPU: nele_asl_p56_var (csrc/level.hip) against vectors generated from the reference's asl_P56 (tests/golden/p56.npz): activity counters
exactly equal, sum of squares to 1e-11, (asl_msq, actfact, c0) to 1e-9 relative, statuses as recorded; batch invariance bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import p56_cases  # noqa: E402

FIELDS = ('asl_msq', 'actfact', 'c0', 'sq', 'counts', 'status')


@pytest.fixture(scope='module')
def golden():
    return p56_cases.load()


def _pad(signals, L=None):
    L = L or max(len(x) for x in signals)
    out = np.zeros((len(signals), L), dtype=np.float32)
    for r, x in enumerate(signals):
        out[r, :len(x)] = x
    return torch.from_numpy(out).cuda(), torch.tensor([len(x) for x in signals], dtype=torch.int32).cuda()


def _host(r):
    torch.cuda.synchronize()
    return {k: r[k].cpu().numpy() for k in FIELDS}


def test_kernel_equals_the_reference_vectors(golden):
    from nele_gan_amd.asl_P56 import batch_asl_P56
    g, cases = golden
    for i, (name, x) in enumerate(cases):
        r = _host(batch_asl_P56(torch.from_numpy(x[None]).cuda()))
        print(name, r['counts'][0].tolist(), r['sq'][0], r['asl_msq'][0], r['actfact'][0], r['c0'][0], r['status'][0])
        assert (r['counts'][0] == g['counts'][i]).all(), (name, r['counts'][0].tolist(), g['counts'][i].tolist())
        assert int(r['status'][0]) == int(g['status'][i]), name
        if float(g['sq'][i]) > 0:
            assert p56_cases.rel(r['sq'][0], g['sq'][i]) <= 1e-11, name
        else:
            assert r['sq'][0] == 0.0
        for k in ('asl_msq', 'actfact', 'c0'):
            if int(g['status'][i]) == 0:
                assert p56_cases.rel(r[k][0], g[k][i]) <= 1e-9, (name, k, r[k][0], float(g[k][i]))
            else:
                assert r[k][0] == 0.0                                      # zeros with the status, never NaN


def test_padded_batch_equals_the_single_utterances_bit_for_bit(golden):
    from nele_gan_amd.asl_P56 import batch_asl_P56
    g, cases = golden
    sig = [x for _, x in cases]
    single = [_host(batch_asl_P56(torch.from_numpy(x[None]).cuda())) for x in sig]
    wav, lens = _pad(sig, 131072)
    wav[:, :] = torch.where(torch.arange(wav.shape[1], device='cuda')[None] < lens[:, None], wav, torch.full_like(wav, 0.25))   # junk behind the rows' ends
    both = _host(batch_asl_P56(wav, lens))
    for i in range(len(sig)):
        for k in FIELDS:
            assert both[k][i].tobytes() == single[i][k][0].tobytes(), (cases[i][0], k)


def test_a_row_is_bit_identical_at_batch_1_50_and_256(golden):
    from nele_gan_amd.asl_P56 import batch_asl_P56
    g, cases = golden
    by = dict(cases)
    row = by['synth_63871']
    others = [by[n][:60000] for n in ('toy_train', 'synth_40000', 'synth_quiet', 'synth_loud', 'synth_16384')]
    one = _host(batch_asl_P56(torch.from_numpy(row[None]).cuda()))
    for B, at in ((50, 17), (256, 201)):
        sig = [others[k % len(others)] for k in range(B)]
        sig[at] = row
        wav, lens = _pad(sig, 64000)
        r = _host(batch_asl_P56(wav, lens))
        for k in FIELDS:
            assert r[k][at].tobytes() == one[k][0].tobytes(), (B, k)
        for k2 in range(B):                                                # and the filler rows equal each other where they repeat
            if k2 != at and k2 >= len(others) and k2 - len(others) != at:
                assert r['counts'][k2].tobytes() == r['counts'][k2 - len(others)].tobytes()


def test_reference_shaped_call(golden):
    from nele_gan_amd.asl_P56 import asl_P56
    g, cases = golden
    for i, (name, x) in enumerate(cases):
        if int(g['status'][i]) == 0:
            if name.startswith('toy') or name == 'synth_quiet':
                got = asl_P56(x, 16000, 16)
                assert all(isinstance(v, float) for v in got)
                for v, k in zip(got, ('asl_msq', 'actfact', 'c0')):
                    assert p56_cases.rel(v, g[k][i]) <= 1e-9
        else:
            with pytest.raises(ValueError, match='NELE_P56_'):
                asl_P56(x, 16000, 16)
