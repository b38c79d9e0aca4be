"""The clean-part protocol of SiibSplit / HaspiSplit / HasqiSplit against a recording cache, on CPU tensors (no GPU: the constructors need
the host-only *_workspace_bytes functions alone, and the library call ``_call`` is replaced by a recorder).

What is pinned: which library calls and which cache calls clean_part() issues, in which order, on which workspace and for which rows,
and what it returns, for a batch that is cached as a whole, in part, not at all, in part with a store that declines, and for a call
that must not touch the cache."""
import pytest
import torch

from nele_gan_amd import metrics as M

B, L, FS = 4, 2400, 16000
KEYS = ['a', 'b', 'c', 'd']
LENGTHS = [2400, 2300, 2200, 2100]
IDS = [11, 12, 13, 14]
HL = [10.0, 20.0, 30.0, 40.0, 50.0, 60.0]


class StubCache:
    """Records every call; ``cached``: the utterance keys it holds; ``decline``: store() stores nothing and says so."""

    def __init__(self, cached=(), decline=False):
        self.index, self.decline, self.log = set(cached), decline, []
        self.partial = 0

    def _slots(self, keys):
        return [('slot', k) for k in keys] if all(k in self.index for k in keys) else None

    def lookup(self, kind, geom, keys, count=True):
        self.log.append(('lookup', kind, geom, list(keys), count))
        return self._slots(keys)

    def missing(self, kind, geom, keys):
        self.log.append(('missing', kind, geom, list(keys)))
        rows = [i for i, k in enumerate(keys) if k not in self.index]
        return rows if 0 < len(rows) < len(keys) else None

    def store(self, kind, geom, ws, nrows, L_, fs, keys):
        self.log.append(('store', kind, geom, ws.data_ptr(), nrows, L_, fs, list(keys)))
        if self.decline:
            return False
        self.index.update(keys)
        return True

    def restore(self, kind, geom, ws, nrows, L_, fs, slots):
        self.log.append(('restore', kind, geom, ws.data_ptr(), nrows, L_, fs, slots))


def _rows(t):
    return None if t is None else t.tolist()


def _x():
    return torch.arange(B, dtype=torch.float32)[:, None].expand(B, L)          # row b holds the value b: a sub-batch shows its rows


DITHER = torch.arange(B, dtype=torch.float64)[:, None] + 100.0


class Case:
    """One split class: how to build it, how to call clean_part, and what a recorded library call looks like."""

    def __init__(self, name):
        self.name = name
        self.kind = name
        self.fs = 0 if name == 'siib' else FS
        self.main, self.sub = name + '_split', name + '_split_sub'

    def make(self, owner, uncacheable=False):
        lengths = torch.tensor(LENGTHS)
        if self.name == 'siib':
            return M.SiibSplit(_x(), lengths=lengths, owner=owner)
        if self.name == 'haspi':
            return M.HaspiSplit(_x(), fs=FS, lengths=lengths, owner=owner)
        if uncacheable:
            return M.HasqiSplit(_x(), fs=FS, lengths=lengths, noise=True, seed=5, HL=HL, owner=owner)
        return M.HasqiSplit(_x(), fs=FS, lengths=lengths, noise='utterance', seed=5, utt_ids=IDS, HL=HL, owner=owner)

    def geom(self, sp):
        if self.name == 'siib':
            return ('L', L)
        if self.name == 'haspi':
            return ('L', L, 'fs', FS, 'dither', 'tag')
        return ('L', L, 'fs', FS, 'noise', (2, 5), 'HL', tuple(HL))

    def clean_part(self, sp, cache, keys, tagged=True):
        if self.name == 'haspi':
            return sp.clean_part(DITHER, cache, keys, 'tag' if tagged else None)
        return sp.clean_part(cache, keys)

    def phase3(self, ws_kind, rows, uncacheable=False):
        """The record of one phase-3 call on workspace ``ws_kind`` for batch rows ``rows``."""
        rec = ('call', 3, ws_kind, [float(r) for r in rows], [LENGTHS[r] for r in rows])
        if self.name == 'haspi':
            return rec + (None, [[100.0 + r] for r in rows])
        if self.name == 'hasqi':
            return rec + (None, (1, 5, HL, None) if uncacheable else (2, 5, HL, [IDS[r] for r in rows]))
        return rec


ALL = pytest.mark.parametrize('name', ['siib', 'haspi', 'hasqi'])


@pytest.fixture
def case(name, monkeypatch):
    c = Case(name)

    def who(sp):
        kind = [k for (k, _dev), t in sp.owner.items() if t is sp.ws]
        assert len(kind) == 1
        return (kind[0], _rows(sp.x[:, 0]), _rows(sp.lengths))

    monkeypatch.setattr(M.SiibSplit, '_call', lambda sp, phase: c.log.append(('call', phase) + who(sp)))
    monkeypatch.setattr(M.HaspiSplit, '_call', lambda sp, y, dither, phase: c.log.append(('call', phase) + who(sp) + (y, _rows(dither))))
    monkeypatch.setattr(M.HasqiSplit, '_call', lambda sp, y, phase, out=None: c.log.append(
        ('call', phase) + who(sp) + (y, (sp.noise, sp.seed, sp.HL, _rows(sp.utt_ids)))))
    return c


def _run(case, cache, keys=KEYS, **kw):
    """-> (split object, owner dict, return value, the one log of library and cache calls in order)"""
    owner = {}
    sp = case.make(owner, uncacheable=kw.pop('uncacheable', False))
    log = case.log = cache.log if cache is not None else []
    ret = case.clean_part(sp, cache, keys, **kw)
    return sp, owner, ret, log


def _ws(owner, kind):
    return owner[(kind, 'cpu')].data_ptr()


@ALL
def test_every_utterance_cached_restores_without_phase_3(case):
    cache = StubCache(KEYS)
    sp, owner, ret, log = _run(case, cache)
    g = case.geom(sp)
    assert ret is True
    assert log == [('lookup', case.kind, g, KEYS, True),
                   ('restore', case.kind, g, _ws(owner, case.main), B, L, case.fs, [('slot', k) for k in KEYS])]
    assert sp.ws is owner[(case.main, 'cpu')] and list(owner) == [(case.main, 'cpu')]
    assert cache.partial == 0


@ALL
def test_some_rows_missing_phase_3_on_a_sub_batch_of_those_rows(case):
    cache = StubCache(['b', 'd'])
    sp, owner, ret, log = _run(case, cache)
    g = case.geom(sp)
    assert ret is True
    assert log == [('lookup', case.kind, g, KEYS, True),
                   ('missing', case.kind, g, KEYS),
                   case.phase3(case.sub, [0, 2]),
                   ('store', case.kind, g, _ws(owner, case.sub), 2, L, case.fs, ['a', 'c']),
                   ('lookup', case.kind, g, KEYS, False),
                   ('restore', case.kind, g, _ws(owner, case.main), B, L, case.fs, [('slot', k) for k in KEYS])]
    assert _ws(owner, case.sub) != _ws(owner, case.main)
    assert cache.partial == 1


@ALL
def test_nothing_cached_phase_3_on_the_batch_then_store(case):
    cache = StubCache()
    sp, owner, ret, log = _run(case, cache)
    g = case.geom(sp)
    assert ret is False
    assert log == [('lookup', case.kind, g, KEYS, True),
                   ('missing', case.kind, g, KEYS),
                   case.phase3(case.main, [0, 1, 2, 3]),
                   ('store', case.kind, g, _ws(owner, case.main), B, L, case.fs, KEYS)]
    assert list(owner) == [(case.main, 'cpu')]
    assert cache.partial == 0


@ALL
def test_a_declined_store_falls_back_to_the_whole_batch(case):
    cache = StubCache(['b', 'd'], decline=True)
    sp, owner, ret, log = _run(case, cache)
    g = case.geom(sp)
    assert ret is False
    assert log == [('lookup', case.kind, g, KEYS, True),
                   ('missing', case.kind, g, KEYS),
                   case.phase3(case.sub, [0, 2]),
                   ('store', case.kind, g, _ws(owner, case.sub), 2, L, case.fs, ['a', 'c']),
                   case.phase3(case.main, [0, 1, 2, 3]),
                   ('store', case.kind, g, _ws(owner, case.main), B, L, case.fs, KEYS)]
    assert cache.partial == 0


@ALL
def test_without_keys_the_cache_is_never_touched(case):
    cache = StubCache(KEYS)
    sp, owner, ret, log = _run(case, cache, keys=None)
    assert ret is False and cache.log == [case.phase3(case.main, [0, 1, 2, 3])]
    sp, owner, ret, log = _run(case, None)
    assert ret is False and log == [case.phase3(case.main, [0, 1, 2, 3])]


@pytest.mark.parametrize('name', ['haspi', 'hasqi'])
def test_what_must_not_be_cached_is_not(case):
    """HASPI with dither rows and no tag that names them; HASQI with noise keyed by the row of the batch."""
    cache = StubCache(KEYS)
    kw = {'tagged': False} if case.name == 'haspi' else {'uncacheable': True}
    sp, owner, ret, log = _run(case, cache, **kw)
    assert ret is False
    assert cache.log == [case.phase3(case.main, [0, 1, 2, 3], uncacheable=True)]
