"""What tests/test_gpu_traj_state.py takes for granted, checked on the CPU for the seeds it uses (tests/traj.py: steps seeded
1000 + k, model seed 5, clip seed 4)."""
import torch

import traj
from traj import B, K

_runs = {}


def _oracle(dtype, opt, plain):
    key = (dtype, opt, plain)
    if key not in _runs:
        masks = []
        _runs[key] = traj.oracle_run(dtype, opt=opt, plain=plain, masks=masks) + (masks,)
    return _runs[key]


def test_two_steps_drop_some_clips_and_not_the_same_ones():
    """Within the K steps at least two steps drop some but not all clips at an FFN, with different patterns: otherwise the
    compaction tables and their pinned upload slots are never re-used with new contents.  The starting seeds do it (steps 1 and
    3: two clips, then one); the dropout-free runs (exact stream, float64 comparison) draw other masks and compact once."""
    assert (traj.STEP_SEED, traj.MODEL_SEED, traj.CLIP_SEED, traj.DROPOUT_P) == (1000, 5, 4, 0.1)
    pats = traj.step_patterns()
    assert len(pats) == K and all(len(p) == traj.LAYERS and all(len(l) == B for l in p) for p in pats)
    partial = [k for k, p in enumerate(pats) if any(0 < sum(l) < B for l in p)]
    assert len(partial) >= 2, pats
    assert len({tuple(map(tuple, pats[k])) for k in partial}) >= 2, 'the partial drops repeat one pattern'
    assert 1 + traj.P * traj.T >= 256, 'clips of fewer than 256 rows never compact'
    assert any(0 < sum(l) < B for p in traj.step_patterns(0.0) for l in p)
    assert traj.step_patterns(0.0) != pats, 'the dropout seed is drawn from the same generator, before the masks'
    lrs, wds = zip(*(traj.schedule('sgd', k) for k in range(K)))
    assert len(set(lrs)) == K and len(set(wds)) == K and min(lrs) > 0, 'lr and weight decay change before every step'


def test_late_joiner_is_outside_the_graph():
    """While it is out, the late joiner's sub-block hands its input on as the very object it got (no kernel, no parameter read, no
    random draw: its DropPath rate is 0); afterwards the class's forward is back."""
    m, _ = traj.build_model(device='cpu')
    mod = traj.late_module(m)
    names = [n for n, _ in mod.named_parameters()]
    assert len(names) == 8 and 'temporal_fc.weight' in names and 'temporal_fc.bias' in names
    assert not mod.layer_drop.dropout_p
    x = torch.zeros(2, 1 + traj.P * traj.T, 128, requires_grad=True)
    traj.set_late(m, True)
    state = torch.get_rng_state()
    y = mod(x)
    assert y is x and torch.equal(torch.get_rng_state(), state)
    y.sum().backward()
    assert all(p.grad is None for p in mod.parameters())
    traj.set_late(m, False)
    assert 'forward' not in mod.__dict__ and mod.forward.__func__ is type(mod).forward
    assert traj.LATE_UNTIL == 2 and K - traj.LATE_UNTIL >= 2


def test_float32_and_float64_oracle_draw_the_same_masks():
    """floor(keep + u) is formed in the working dtype: the float32 and the float64 oracle trajectories must keep the same
    sequences, and the FFN's are the ones the float32 predictor (the arithmetic of transformer.DropPath) gives."""
    m64, m32 = _oracle(torch.float64, 'sgd', False)[3], _oracle(torch.float32, 'sgd', False)[3]
    assert len(m64) == len(m32) == 3 * (traj.LAYERS - 1) * K
    assert all(torch.equal(a, b) for a, b in zip(m64, m32))
    pats = traj.step_patterns(0.0)
    for k in range(K):
        assert [not v for v in m64[3 * k + 2].tolist()] == pats[k][1], k


def test_float32_yardstick_and_adamw_conditioning():
    """The oracle in float32 against itself in float64 after K steps, per parameter tensor (relative L2).  With torch.optim alone
    (no clipping, no decay) SGD(lr 0.02) gives 9.4e-7 on its worst tensor -- the recorded yardstick, held here within a factor
    of 2 -- and AdamW(lr 1e-3) 3.4e-2, 0.35 of that tensor's own travel: above 1e-2, which is why the float64 comparison leaves
    AdamW out.  The stack's own SGD trajectory (clipping, decay, schedule) is as well conditioned: 3.8e-6 of the distance travelled."""
    recorded = 9.4e-7
    p64, _, start, _ = _oracle(torch.float64, 'sgd', True)
    worst, name = traj.worst_tensor(_oracle(torch.float32, 'sgd', True)[0], p64)
    print(f'SGD float32 vs float64: worst tensor {worst:.3e} ({name})')
    assert recorded / 2 <= worst <= recorded * 2, worst
    s64, _, s_start, _ = _oracle(torch.float64, 'sgd', False)
    d = traj.drift(_oracle(torch.float32, 'sgd', False)[0], s64, s_start)
    print(f'the stack\'s SGD trajectory, float32 vs float64: {d:.3e} of the distance travelled')
    assert d <= 2 * 3.8e-6, d
    a64, _, a_start, _ = _oracle(torch.float64, 'adamw', True)
    a32 = _oracle(torch.float32, 'adamw', True)[0]
    cond, cname = traj.worst_own_travel(a32, a64, a_start)
    print(f'AdamW float32 vs float64: worst tensor {traj.worst_tensor(a32, a64)[0]:.3e}; {cond:.3e} of its own travel ({cname})')
    assert cond > 1e-2, cond
