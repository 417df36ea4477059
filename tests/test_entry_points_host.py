"""The public entry points of ``lts_array`` and ``narrow_band_least_squares`` against a stand-in engine
(tests/entry_point_cases.py): a batch form is its single form per recording, a batch of one IS the single call, an empty
batch touches nothing, the message of an ordinary least squares fit prints once, every entry point passes the engine the
keywords it always passed, and the narrow-band entry points refuse a bad ALPHA and mismatched response rows in the words
they always used.  CPU only, no GPU library."""
import numpy as np
import pytest

import entry_point_cases as ep

BATCHED = sorted(name for name, case in ep.PAIRS.items() if case[1] is not None)


def _same(a, b, where=''):
    """Field by field: the same types, tuple lengths and dictionary keys, arrays equal with dtype and shape (NaN = NaN)."""
    assert type(a) is type(b), where
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (where, i))
    elif isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for k in a:
            _same(a[k], b[k], '%s[%r]' % (where, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, where
        assert np.array_equal(a, b, equal_nan=a.dtype.kind in 'fc'), where
    else:
        assert a == b or (a != a and b != b), where


def _aliases(x, results):
    pool = [a for res in results for a in res.__dict__.values() if isinstance(a, np.ndarray)]
    return any(np.shares_memory(x, a) for a in pool)


@pytest.mark.parametrize('alpha', [1.0, 0.75])
@pytest.mark.parametrize('name', BATCHED)
def test_a_batch_is_the_single_call_per_recording(name, alpha, capsys):
    single, batch = ep.PAIRS[name][:2]
    with ep.stand_in() as s:
        one = single(ep.stream(), alpha)
    assert s.names() == ['process']
    said = capsys.readouterr().out
    with ep.stand_in() as s:
        three = batch([ep.stream(), ep.stream(), ep.stream()], alpha)
    assert s.names() == ['process_batch']
    assert capsys.readouterr().out == said
    assert said.count(ep.OLS_MESSAGE) == (1 if alpha == 1.0 and name.startswith('ltsva') else 0)
    assert isinstance(three, list) and len(three) == 3
    for i, element in enumerate(three):
        _same(element, one, '%s, recording %d' % (name, i))


@pytest.mark.parametrize('alpha', [1.0, 0.75])
@pytest.mark.parametrize('name', BATCHED)
def test_a_batch_of_one_is_the_single_call(name, alpha, capsys):
    single, batch = ep.PAIRS[name][:2]
    with ep.stand_in() as s:
        one = single(ep.stream(), alpha)
    single_call = s.calls[0]
    said = capsys.readouterr().out
    with ep.stand_in() as s:
        out = batch([ep.stream()], alpha)
    assert s.names() == ['process']                                  # not process_batch, and once
    assert sorted(s.calls[0][2]) == sorted(single_call[2])           # with the single call's keywords, callbacks included
    assert capsys.readouterr().out == said                           # the message once, not twice
    assert len(out) == 1
    _same(out[0], one, name)


@pytest.mark.parametrize('name', BATCHED)
def test_an_empty_batch_touches_nothing(name, capsys):
    with ep.stand_in() as s:
        assert ep.PAIRS[name][1]([], 1.0) == []
        assert ep.PAIRS[name][1](iter(()), 0.75) == []
    assert s.calls == [] and capsys.readouterr().out == ''


@pytest.mark.parametrize('name', sorted(ep.PAIRS))
def test_the_keywords_the_engine_gets(name):
    single, batch, process_kw, batch_kw = ep.PAIRS[name]
    told = ep._NB_TOLD if name.startswith('narrow_band') else ep._TOLD
    with ep.stand_in() as s:
        single(ep.stream(), 0.75)
        if batch is not None:
            batch([ep.stream(), ep.stream(0.01)], 0.75)
    assert set(s.calls[0][2]) == process_kw | told
    if batch is not None:
        assert s.calls[1][0] == 'process_batch' and set(s.calls[1][2]) == batch_kw


@pytest.mark.parametrize('name', sorted(ep.NARROW_BAND))
def test_the_keywords_of_the_narrow_band_entry_points(name):
    with ep.stand_in() as s:
        ep.NARROW_BAND[name][0](ep.stream(), 0.75)
    assert s.names() == ['process'] and set(s.calls[0][2]) == ep.NARROW_BAND[name][1] | ep._NB_TOLD


def _arrays(x):
    if isinstance(x, np.ndarray):
        yield x
    elif isinstance(x, (tuple, list, dict)):
        for v in (x.values() if isinstance(x, dict) else x):
            yield from _arrays(v)


@pytest.mark.parametrize('name', sorted(n for n in ep.PAIRS if n.startswith('ltsva')))
def test_every_ltsva_form_returns_copies(name):
    single, batch = ep.PAIRS[name][:2]
    with ep.stand_in() as s:
        out = [single(ep.stream(), 0.75)] + (batch([ep.stream(), ep.stream()], 0.75) if batch is not None else [])
    arrays = list(_arrays(out))
    assert len(arrays) >= 7 * len(out) and not any(_aliases(a, s.results) for a in arrays)


def test_the_single_forms_return_copies_and_the_narrow_band_forms_the_rows_themselves():
    with ep.stand_in() as s:
        out = ep.PAIRS['ltsva_kept'][0](ep.stream(), 0.75)
    nwin = int(s.results[0].nwin[0])
    for a in out[:4] + out[5:8] + tuple(out[8].values()):
        assert len(a) == nwin and not _aliases(a, s.results)
    with ep.stand_in() as s:
        out = ep.NARROW_BAND['narrow_band_least_squares_capon'][0](ep.stream(), 1.0)
    res = s.results[0]
    assert out[0] is res.vel and out[1] is res.baz and out[2] is res.mdccm and out[3] is res.t and out[5] is res.sigma_tau
    assert out[9]['capon_power'] is res.capon_power and out[9]['capon_index'] is res.capon_index
    beyond = np.arange(res.vel.shape[1])[None, :] >= np.asarray(res.nwin)[:, None]
    assert beyond.any() and not out[9]['capon_vel'][beyond].any() and not out[9]['bartlett_baz'][beyond].any()
    assert out[9]['capon_vel'][~beyond].all()


@pytest.mark.parametrize('name', sorted(ep.NARROW_BAND))
def test_a_bad_alpha_and_mismatched_response_rows(name):
    call, _, has_range = ep.NARROW_BAND[name]
    with ep.stand_in() as s:
        if has_range:
            with pytest.raises(ValueError) as e:
                call(ep.stream(), 0.3)
            assert str(e.value) == ep.ALPHA_MESSAGE
        with pytest.raises(ValueError) as e:
            call(ep.stream(), 1.0, rows=7)
        assert str(e.value) == ep.RESPONSE_MESSAGE
    assert s.calls == []


@pytest.mark.parametrize('name', ['narrow_band_least_squares', 'narrow_band_least_squares_families'])
def test_mismatched_response_rows_in_a_batch(name):
    with ep.stand_in() as s:
        for streams in ([ep.stream()], [ep.stream(), ep.stream()]):
            with pytest.raises(ValueError) as e:
                ep.PAIRS[name][1](streams, 1.0, rows=7)
            assert str(e.value) == ep.RESPONSE_MESSAGE
    assert s.calls == []


@pytest.mark.parametrize('name', sorted(ep.VALUES))
def test_the_values_of_some_keywords(name):
    single, batch = ep.PAIRS[name][:2] if name in ep.PAIRS else (ep.NARROW_BAND[name][0], None)
    with ep.stand_in() as s:
        single(ep.stream(), 0.75)
        if batch is not None:
            batch([ep.stream(), ep.stream(0.01)], 0.75)
    for call in s.calls:
        for k, v in ep.VALUES[name].items():
            if k in call[2] or call[0] == 'process':
                assert type(call[2][k]) is type(v) and call[2][k] == v, (call[0], k)
