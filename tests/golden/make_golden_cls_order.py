"""Goldens of the space-then-time operator order from the UNMODIFIED reference (dev container only: needs the reference):

    python tests/golden/make_golden_cls_order.py

operator_order = ['space_attn', 'time_attn', 'ffn']: the spatial block runs without the cls token, the temporal block over it
(reference transformer.py:602,611).  Every case is a TransformerContainer of head_dim 64 (embed_dims 128, 2 heads, hidden 256)
run on the CPU in fp32.  The weights are oracle.synth.synth_state_dict(shapes, seed); the input is
numpy.random.RandomState(seed).standard_normal -- the tests rebuild both, the files hold outputs and gradients only.

  cls_order_<case>.npz     'out' (whole, or 'outs' = helpers.NS strided samples of a large one), per parameter 'g:' (whole) or
                           'gs:' + 'gn:' (NS strided samples + norm and sum), 'attn' for the return_attention case.
  cls_order_cal.json       per case: the deviation of the reference's own torch.autocast(bfloat16) run from its fp32 run, 'out' in
                           the metric of helpers.relerr and 'grad' per tensor in the metric of helpers.compare_grads.

Train cases draw DropPath from the CPU default generator after torch.manual_seed(seed); loss = sum(out * w), w =
10 * synth_tensor('loss_w', (D,), 0).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import ref_loader, synth  # noqa: E402
from helpers import NS, relerr, sample_idx  # noqa: E402

ORDER = ['space_attn', 'time_attn', 'ffn']
D, HEADS, HIDDEN = 128, 2, 256
# name: (clips, T, P, layers, drop_path_rate, mode)
CASES = {
    't8_p16': (2, 8, 16, 1, 0.0, 'train'),            # both blocks in the <= 32-token family
    't8_p196': (1, 8, 196, 1, 0.0, 'train'),          # spatial 196, temporal 9: the TimeSformer-B geometry at reduced width
    't32_p16': (2, 32, 16, 1, 0.0, 'train'),          # temporal 33
    't8_p16_eval_attn': (2, 8, 16, 2, 0.0, 'eval'),   # eval + return_attention
    't8_p16_droppath': (4, 8, 16, 2, 0.3, 'train'),   # two layers, DropPath drawn after manual_seed
}
SEED = {name: 11 + i for i, name in enumerate(CASES)}


def make_input(name):
    B, T, P = CASES[name][:3]
    return torch.from_numpy(np.random.RandomState(SEED[name]).standard_normal((B, 1 + P * T, D)).astype(np.float32))


def build(TR, name):
    B, T, P, layers, dpr, mode = CASES[name]
    m = TR.TransformerContainer(num_transformer_layers=layers, embed_dims=D, num_heads=HEADS, num_frames=T,
                                hidden_channels=HIDDEN, operator_order=list(ORDER), drop_path_rate=dpr)
    m.load_state_dict(synth.synth_state_dict(synth.shapes_of(m), SEED[name]), strict=True)
    return m


def run(m, x, name, autocast):
    mode = CASES[name][5]
    res = {}
    ctx = torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast)
    if mode == 'eval':
        m.eval()
        with torch.no_grad(), ctx:
            res['out'] = m(x).float()
            res['attn'] = m(x, return_attention=True).float()
        return res, {}
    m.train()
    m.zero_grad()
    torch.manual_seed(SEED[name])
    with ctx:
        y = m(x).float()
    w = synth.synth_tensor('loss_w', (D,), 0) * 10.0
    (y * w).sum().backward()
    res['out'] = y.detach()
    return res, {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def grad_dev(got, ref):
    """helpers.compare_grads' relative L2 error of one tensor, for the stored form of that tensor."""
    got, ref = got.double().flatten(), ref.double().flatten()
    if ref.numel() <= NS:
        return float((got - ref).norm() / max(float(ref.norm()), 1e-30))
    idx = sample_idx(ref.numel())
    rms = float(ref.norm()) / ref.numel() ** 0.5
    ref_norm = max(float(ref[idx].norm()), rms * idx.numel() ** 0.5)
    norm_err = abs(float(got.norm()) - float(ref.norm())) / max(float(ref.norm()), 1e-30)
    return max(float((got[idx] - ref[idx]).norm()) / max(ref_norm, 1e-30), norm_err)


def main():
    TR = ref_loader.load().transformer
    torch.set_num_threads(min(16, os.cpu_count()))
    cal = {}
    for name in CASES:
        m, x = build(TR, name), make_input(name)
        res, grads = run(m, x, name, False)
        ac, ac_grads = run(m, x, name, True)
        out = {}
        for k, v in res.items():
            flat = v.flatten()
            if k == 'out' and flat.numel() > 16 * NS:
                out['outs'] = flat[sample_idx(flat.numel())].numpy()
            else:
                out[k] = v.numpy()
        for k, g in grads.items():
            flat = g.flatten()
            if flat.numel() <= NS:
                out['g:' + k] = g.numpy()
            else:
                out['gs:' + k] = flat[sample_idx(flat.numel())].numpy()
                out['gn:' + k] = np.array([float(g.double().norm()), float(g.double().sum())])
        np.savez_compressed(os.path.join(HERE, f'cls_order_{name}.npz'), **out)
        cal['cls_order ' + name] = {'out': relerr(ac['out'], res['out']),
                                    'grad': {k: grad_dev(ac_grads[k], grads[k]) for k in grads}}
        if 'attn' in res:
            cal['cls_order ' + name]['attn'] = relerr(ac['attn'], res['attn'])
        gd = sorted(cal['cls_order ' + name]['grad'].values())
        print(name, {k: v.shape for k, v in out.items() if not k.startswith('g')}, 'autocast out', f"{cal['cls_order ' + name]['out']:.3e}",
              'grad median / worst', f'{gd[len(gd) // 2]:.3e} / {gd[-1]:.3e}' if gd else '-', flush=True)
    json.dump(cal, open(os.path.join(HERE, 'cls_order_cal.json'), 'w'), indent=0, sort_keys=True)


if __name__ == '__main__':
    main()
