"""Host-side checks of the hand-off between sub-blocks under the exact residual stream (no GPU, libvtx.so is not loaded):
transformer._stream_of and stream_value look at types, dtypes and the mode only; a Stream is not usable as a tensor; VTX_STREAM
takes the values of vtx.set_stream and nothing else."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import ROOT

PKG = os.path.join(ROOT, 'videotransformer-pytorch_amd')

MODES = ['bf16', 'fp32', 'fp32+grad']


@pytest.fixture
def stream_mode():
    """set(mode) -> vtx.set_stream; the mode is put back whatever the case does."""
    import vtx
    before = vtx.get_stream()
    try:
        yield vtx.set_stream
    finally:
        vtx.set_stream(before)


def _pair():
    return torch.zeros(2, 3, 8, dtype=torch.bfloat16), torch.zeros(2, 3, 8)


@pytest.mark.parametrize('mode', MODES)
def test_stream_of_a_plain_tensor(stream_mode, mode):
    """float32 activations are their own exact stream in every mode; a bf16 tensor is the bf16 stream with the mode off and the
    START of the float32 stream (no xs yet) with it on."""
    import transformer as T_
    stream_mode(mode)
    d, xs = _pair()
    d0, x0, exact = T_._stream_of(xs)
    assert d0 is xs and x0 is None and exact is False
    d0, x0, exact = T_._stream_of(d)
    assert d0 is d and x0 is None and exact is (mode != 'bf16')


@pytest.mark.parametrize('mode', ['fp32', 'fp32+grad'])
def test_stream_of_a_stream(stream_mode, mode):
    import transformer as T_
    stream_mode(mode)
    d, xs = _pair()
    d0, x0, exact = T_._stream_of(T_.Stream(d, xs))
    assert d0 is d and x0 is xs and exact is True
    d0, x0, exact = T_._stream_of(T_.Stream(d, None))
    assert d0 is d and x0 is None and exact is True


def test_a_stream_with_the_mode_off_is_a_caller_error(stream_mode):
    import transformer as T_
    stream_mode('bf16')
    d, xs = _pair()
    with pytest.raises(TypeError):
        T_._stream_of(T_.Stream(d, xs))


@pytest.mark.parametrize('mode', MODES)
def test_stream_value_of_what_is_already_one_tensor(stream_mode, mode):
    import transformer as T_
    stream_mode(mode)
    d, xs = _pair()
    assert T_.stream_value(d) is d
    assert T_.stream_value(xs) is xs
    assert T_.stream_value(T_.Stream(d, None)) is d


def test_with_stream_builds_the_pair_in_exact_mode_only():
    import transformer as T_
    d, xs = _pair()
    s = T_._with_stream((d, xs), True)
    assert type(s) is T_.Stream and s.d is d and s.xs is xs
    assert T_._with_stream(d, False) is d


@pytest.mark.parametrize('method', ['clone', 'float', 'contiguous', 'detach', 'to'])
def test_a_stream_is_not_usable_as_a_tensor(method):
    """What used to drop the float32 stream without a word now raises."""
    import transformer as T_
    s = T_.Stream(*_pair())
    with pytest.raises(AttributeError):
        getattr(s, method)
    assert not isinstance(s, torch.Tensor)


def _import_vtx(value):
    env = {k: v for k, v in os.environ.items() if k != 'VTX_STREAM'}
    if value is not None:
        env['VTX_STREAM'] = value
    code = f'import sys; sys.path.insert(0, {PKG!r}); import vtx; print(vtx.get_stream())'
    return subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True)


@pytest.mark.parametrize('value', ['FP32', 'fp32_grad', 'exact'])
def test_a_misspelt_vtx_stream_fails_the_import(value):
    r = _import_vtx(value)
    assert r.returncode != 0 and 'ValueError' in r.stderr, (r.returncode, r.stderr[-400:])


@pytest.mark.parametrize('value,mode', [('fp32+grad', 'fp32+grad'), (None, 'bf16')])
def test_a_valid_or_unset_vtx_stream_imports_cleanly(value, mode):
    r = _import_vtx(value)
    assert r.returncode == 0, r.stderr[-400:]
    assert r.stdout.strip().endswith(mode)
