"""Multi-step training trajectories of the product's training stack (helper, no test functions).

What ``bench.py`` and ``model_pretrain.Trainer._train_step`` run -- ``vtx.dp.GradBuckets(direct=True)`` with ``zero()`` /
``finish()`` around the backward, DropPath-aware FFN compaction, the merged attn.proj o temporal_fc projection, a fused optimizer
with per-parameter clipping over a no-decay / decay pair of groups, a schedule that rewrites ``lr`` (both groups) and
``weight_decay`` (the decayed group) before every step -- over K steps on a tiny model, in several ARMS that differ only in how
much state they carry from one step to the next.  Every kernel is deterministic and every random draw comes from the CPU default
generator, so all arms must agree BIT FOR BIT (tests/test_gpu_traj_state.py); the same schedule on the CPU oracle in float64 is
the yardstick of tests/test_gpu_traj_state.py's float64 part and of tests/test_traj_premise.py.

Model: TimeSformer divided_space_time, 4 clips of 16 frames of 64 x 64, patch 16, D 128, 2 heads, 2 layers: 1 + 16 * 16 = 257
rows per clip, the smallest shape at which the FFN compaction and its table upload run at all (rows_per >= 256).

Dropout.  The drop-in models take ONE dropout argument, ``dropout_p`` (drop_after_pos / drop_after_time); it is 0.1 here, so every
training forward draws one dropout seed before the DropPath masks.  The blocks' ``proj_drop`` and the FFN's ``dropout_p`` have no
constructor argument in the models (as in the reference), and switching them on by hand turns the merged projection and the FFN
compaction OFF (a mask sits inside them: vtx.functions.TimeAttnFn / FFNFn) -- the very state this file is about.  ``block_drop``
sets them by hand for the arms that say so.  The exact residual stream (vtx.set_stream('fp32')) refuses embedding dropout, so
the arms under it run with ``dropout_p`` 0."""
import copy
import gc

import numpy as np
import torch

from oracle import synth, vt_oracle as O

DEV = 'cuda:0'
K = 4
MODEL_SEED, CLIP_SEED, STEP_SEED = 5, 4, 1000
B, T, IMG, PATCH, HEADS, LAYERS = 4, 16, 64, 16, 2, 2
P = (IMG // PATCH) ** 2
DROP_PATH = 0.1
DROPOUT_P = 0.1
CLIP_GRAD = 0.5
WEIGHT_DECAY = 0.05
BASE_LR = {'sgd': 0.02, 'adamw': 1e-3}
LATE_UNTIL = 2                       # the late joiner's sub-block is outside the graph in steps 0 .. LATE_UNTIL - 1


def schedule(opt, k):
    """(lr of both groups, weight_decay of the decayed group) before step k: both change at every step."""
    return BASE_LR[opt] * (1.0 - 0.15 * k), WEIGHT_DECAY * (1.0 + 0.5 * k)


def ffn_drop_pattern(seed, B, P, T, layers, rate=0.1, seed_draws=0):
    """The FFN DropPath masks a training forward draws after torch.manual_seed(seed): per layer with p > 0 the reference draws
    (B*P) temporal, (B*T) spatial and B FFN values from the CPU generator, in that order (transformer.py:34-42, 268-275, 371-377, 543).
    seed_draws: dropout seeds (transformer._draw_seed) the forward draws before the first block -- one with embedding dropout on."""
    torch.manual_seed(seed)
    for _ in range(seed_draws):
        torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)
    out = []
    for p in np.linspace(0, rate, layers):
        if p == 0:
            out.append([False] * B)
            continue
        torch.rand(B * P, 1, 1)
        torch.rand(B * T, 1, 1)
        u = torch.rand(B, 1, 1).reshape(B)
        out.append([bool(np.floor(np.float32(1 - p) + np.float32(v)) == 0) for v in u.tolist()])
    return out


def step_patterns(dropout_p=DROPOUT_P):
    """Per step of the trajectory: the dropped clips of every layer's FFN."""
    return [ffn_drop_pattern(STEP_SEED + k, B, P, T, LAYERS, DROP_PATH, seed_draws=1 if dropout_p else 0) for k in range(K)]


def seed_step(k):
    torch.manual_seed(STEP_SEED + k)
    np.random.seed(STEP_SEED + k)


# ---------------------------------------------------------------------------------------------------------------- models
def model_cfg(model='tsf', D=128):
    cfg = dict(num_frames=T, img_size=IMG, patch_size=PATCH, embed_dims=D, num_heads=HEADS, num_transformer_layers=LAYERS)
    if model == 'vivit':
        cfg.update(attention_type='fact_encoder', conv_type='Conv3d', tube_size=2)
    return cfg


def build_model(model='tsf', D=128, seed=MODEL_SEED, dropout_p=DROPOUT_P, block_drop=0.0, device=DEV):
    import transformer as T_
    import video_transformer as V
    m = (V.ViViT if model == 'vivit' else V.TimeSformer)(dropout_p=dropout_p, **model_cfg(model, D))
    sd = synth.synth_state_dict(synth.shapes_of(m), seed)
    m.load_state_dict(sd, strict=True)
    if block_drop:
        for mod in m.modules():
            if isinstance(mod, T_.FFNWithPreNorm):
                mod.dropout_p = block_drop
            elif hasattr(mod, 'proj_drop') and hasattr(mod, 'layer_drop'):
                mod.proj_drop.p = block_drop
    return m.to(device).train(), sd


def data(D=128, model='tsf'):
    """(training clips, held-out clips, target) on the CPU."""
    x = synth.synth_clip(B, T, 3, IMG, IMG, seed=CLIP_SEED)
    xh = synth.synth_clip(2, T, 3, IMG, IMG, seed=CLIP_SEED + 50)
    tgt = synth.synth_tensor('target', (B, D), MODEL_SEED) * 0.5
    return x, xh, tgt


def param_groups(named):
    """[no-decay group, decayed group] by optimizer.py's rule: vectors, biases, pos_embed and cls_token take no decay."""
    plain = lambda k, p: p.ndim == 1 or k.endswith('.bias') or any(w in k for w in ('pos_embed', 'cls_token', 'mask_token'))      # noqa: E731
    nd = [p for k, p in named if plain(k, p)]
    dec = [p for k, p in named if not plain(k, p)]
    return [dict(params=nd, weight_decay=0.0), dict(params=dec, weight_decay=WEIGHT_DECAY)]


def late_module(m):
    """The late joiner: the temporal attention sub-block of layer 0 (norm, qkv, proj and temporal_fc).  Its DropPath rate is
    0, so leaving it out moves no random draw."""
    return m.transformer_layers.layers[0].attentions[0]


def set_late(m, out):
    """out=True: the sub-block hands its input on untouched -- its parameters are outside the graph; False: it joins."""
    mod = late_module(m)
    if out:
        mod.forward = lambda query, *a, **kw: query
    else:
        mod.__dict__.pop('forward', None)


# ------------------------------------------------------------------------------------------------------------ the GPU run
def make_optimizer(opt, m):
    from vtx import optim
    groups = param_groups(list(m.named_parameters()))
    if opt == 'sgd':
        return optim.FusedSGD(groups, lr=BASE_LR[opt], momentum=0.9, nesterov=True, weight_decay=WEIGHT_DECAY, clip_grad=CLIP_GRAD)
    return optim.FusedAdamW(groups, lr=BASE_LR[opt], weight_decay=WEIGHT_DECAY, clip_grad=CLIP_GRAD)


class Traj:
    """One model, its buckets and optimizer, stepped by ``step(k)``; ``result()`` brings everything to the CPU.

    cold: nothing is carried -- clear_weight_cache() before every forward, fresh GradBuckets every step (the old one
          remove()d), before every optimizer step a fresh fused optimizer loaded from a deepcopy of the previous one's
          state_dict(), torch.cuda.synchronize() after every step.  Otherwise ("warm") the host never waits for the device.
    precs: the precision of step k is precs[k % len(precs)].
    late:  late_module() is outside the graph in steps 0 .. LATE_UNTIL - 1 (set_skipped(buckets.unfired()) keeps its update away).
    evals: after every step one eval forward under no_grad on the held-out clips and one training-mode forward whose graph is
           dropped; the eval outputs and device clones of the weights they ran on are kept.
    fresh_buckets: new GradBuckets before every step UNDER THE LIVE OPTIMIZER; the old ones are removed but kept alive, so the
           new gradient views cannot land on the old addresses."""

    def __init__(self, prec='bf16', opt='sgd', model='tsf', D=128, seed=MODEL_SEED, cold=False, stream='bf16', precs=None,
                 late=False, evals=False, dropout_p=DROPOUT_P, block_drop=0.0, recompute=False, fresh_buckets=False):
        from vtx import dp
        self.precs = list(precs) if precs else [prec]
        self.optname, self.cold, self.stream, self.late, self.evals, self.recompute = opt, cold, stream, late, evals, recompute
        self.kind = dict(model=model, D=D, dropout_p=dropout_p, block_drop=block_drop)
        self.model, self.start = build_model(seed=seed, **self.kind)
        x, xh, tgt = data(D, model)
        self.x, self.xh, self.tgt = x.to(DEV), xh.to(DEV), tgt.to(DEV)
        self.buckets = dp.GradBuckets(list(self.model.parameters()), direct=True)
        self.opt = make_optimizer(opt, self.model)
        self.losses, self.eval_out, self.eval_weights = [], [], []
        self.fresh_buckets, self.old_buckets = fresh_buckets, []

    def _modes(self, k):
        import vtx
        vtx.set_precision(self.precs[k % len(self.precs)])
        vtx.set_stream(self.stream)
        vtx.set_recompute(self.recompute)

    def step(self, k):
        from vtx import dp, functions
        self._modes(k)
        lr, wd = schedule(self.optname, k)
        for g in self.opt.param_groups:
            g['lr'] = lr
        self.opt.param_groups[1]['weight_decay'] = wd
        seed_step(k)
        if self.cold:
            functions.clear_weight_cache()
            self.buckets.remove()
            self.buckets = dp.GradBuckets(list(self.model.parameters()), direct=True)
        elif self.fresh_buckets:
            self.buckets.remove()
            self.old_buckets.append(self.buckets)
            self.buckets = dp.GradBuckets(list(self.model.parameters()), direct=True)
        if self.late:
            set_late(self.model, k < LATE_UNTIL)
        self.buckets.zero()
        y = self.model(self.x)
        loss = 0.5 * ((y - self.tgt) ** 2).sum()
        loss.backward()
        self.buckets.finish()
        if self.cold:
            fresh = make_optimizer(self.optname, self.model)
            fresh.load_state_dict(copy.deepcopy(self.opt.state_dict()))
            self.opt = fresh
        self.opt.set_skipped(self.buckets.unfired())
        self.opt.step()
        self.losses.append(loss.detach())
        if self.evals:
            self.model.eval()
            with torch.no_grad():
                self.eval_out.append(self.model(self.xh))
            self.model.train()
            self.model(self.x)                                   # a training-mode forward whose graph is dropped
            self.eval_weights.append({n: v.detach().clone() for n, v in self.model.state_dict().items()})
        if self.cold:
            torch.cuda.synchronize()

    def reload_in_place(self):
        """optimizer.load_state_dict of its own (deep-copied) state: new state tensors under the same optimizer object."""
        self.opt.load_state_dict(copy.deepcopy(self.opt.state_dict()))

    def restore_in_place(self, path):
        """Both state dicts loaded into the LIVE objects (a roll-back): Module.load_state_dict is a versioned copy_ into the very
        parameters whose staged copies sit in the weight cache, and nobody clears it."""
        state = torch.load(path, map_location='cpu')
        self.model.load_state_dict(state['model'])
        self.opt.load_state_dict(state['optimizer'])

    def save(self, path):
        torch.save({'model': self.model.state_dict(), 'optimizer': self.opt.state_dict()}, path)

    @classmethod
    def resumed(cls, path, losses, clear=False, **kw):
        """New objects with ANOTHER initialisation, both state dicts loaded from the file.  Module.load_state_dict is a versioned
        copy_: the weight cache must notice by itself (clear=False)."""
        from vtx import functions
        self = cls(seed=MODEL_SEED + 1, **kw)
        state = torch.load(path, map_location='cpu')
        self.model.load_state_dict(state['model'])
        self.opt.load_state_dict(state['optimizer'])
        if clear:
            functions.clear_weight_cache()
        self.losses = list(losses)
        return self

    def result(self):
        torch.cuda.synchronize()
        names = {id(p): n for n, p in self.model.named_parameters()}
        order = [names[id(p)] for g in self.opt.param_groups for p in g['params']]
        sd = self.opt.state_dict()
        state, steps = {}, {}
        for i, st in sd['state'].items():
            steps[order[i]] = int(float(st['step']))
            state[order[i]] = {key: v.detach().cpu().clone() for key, v in st.items() if key != 'step' and torch.is_tensor(v)}
        return dict(losses=torch.stack([l.float() for l in self.losses]).cpu(),
                    params={n: v.detach().cpu().clone() for n, v in self.model.state_dict().items()},
                    state=state, steps=steps, evals=[e.cpu() for e in self.eval_out])

    def close(self):
        import vtx
        if self.late:
            set_late(self.model, False)
        self.buckets.remove()
        vtx.set_precision('auto')
        vtx.set_stream('bf16')
        vtx.set_recompute(False)

    def drop(self):
        """Let go of the model, optimizer and buckets (their ids and allocations may be recycled)."""
        self.close()
        self.model = self.opt = self.buckets = None
        self.old_buckets = []
        self.eval_weights = []
        gc.collect()


def run(arm='warm', steps=K, resume_at=None, path=None, clear=False, reload_at=None, rollback_at=None, **kw):
    """The K-step trajectory of one arm -> result() (losses, parameters, optimizer state tensors and step counts, on the CPU).
    arm: 'warm' | 'cold'.  resume_at: after that many steps save to ``path``, drop everything, continue in new objects.
    reload_at: after that many steps the optimizer reloads its own state dict in place.
    rollback_at: after that many steps save to ``path``, take one more step, throw it away by loading the file into the live
    objects, and go on from there."""
    t = Traj(cold=(arm == 'cold'), **kw)
    try:
        for k in range(steps):
            if resume_at is not None and k == resume_at:
                t.save(path)
                losses = t.losses
                t.drop()
                t = Traj.resumed(path, losses, clear=clear, cold=(arm == 'cold'), **kw)
            if rollback_at is not None and k == rollback_at:
                t.save(path)
                t.step(k)
                t.losses.pop()
                t.restore_in_place(path)
            if reload_at is not None and k == reload_at:
                t.reload_in_place()
            t.step(k)
        return t.result()
    finally:
        t.close()


def cold_eval(weights, xh, **kind):
    """The eval output of a cold model holding ``weights``: a new model, no staged weight copy anywhere."""
    from vtx import functions
    m, _ = build_model(seed=MODEL_SEED + 2, **kind)
    m.load_state_dict(weights)
    functions.clear_weight_cache()
    m.eval()
    with torch.no_grad():
        y = m(xh)
    functions.clear_weight_cache()
    return y.cpu()


def diff(a, b):
    """Everything in which two result() dicts differ in any bit: [] when the two runs are the same trajectory."""
    out = []
    if not torch.equal(a['losses'], b['losses']):
        out.append('losses: %s vs %s' % (a['losses'].tolist(), b['losses'].tolist()))
    for what in ('params', 'state'):
        if sorted(a[what]) != sorted(b[what]):
            out.append(f'{what}: different keys {sorted(set(a[what]) ^ set(b[what]))}')
            continue
        for n in a[what]:
            u, v = a[what][n], b[what][n]
            if what == 'params':
                u, v = {'': u}, {'': v}
            if sorted(u) != sorted(v):
                out.append(f'{what} {n}: different entries')
                continue
            for key in u:
                if not torch.equal(u[key], v[key]):
                    out.append(f'{what} {n} {key}: {(u[key] != v[key]).sum().item()} of {u[key].numel()} elements differ')
    if a['steps'] != b['steps']:
        out.append('step counts: %s' % sorted((n, a['steps'].get(n), b['steps'].get(n)) for n in set(a['steps']) | set(b['steps'])
                                             if a['steps'].get(n) != b['steps'].get(n)))
    return out


# -------------------------------------------------------------------------------------------------------- the CPU oracle
def oracle_run(dtype=torch.float64, autocast=False, opt='sgd', steps=K, masks=None, plain=False):
    """The same K steps on oracle/vt_oracle.timesformer_forward with torch.optim (CPU): the clipping rule of the fused step
    (per parameter, by its own norm: coef = clip / (norm + 1e-6) when that is below 1), the same groups and schedule, DropPath
    on with the same draws, no dropout (the oracle has none: compare with dropout_p=0 runs).  -> (parameters, losses, start).
    masks: a list that receives every DropPath keep mask drawn (one bool tensor per draw).
    plain: torch.optim alone -- no clipping, no weight decay (the optimizers whose float32 rounding the issue's table records)."""
    sd0 = synth.synth_state_dict(synth.shapes_of(build_model(device='cpu')[0]), MODEL_SEED)
    ps = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd0.items()}
    x, _, tgt = data()
    groups = param_groups(list(ps.items()))
    decay = 0.0 if plain else 1.0
    if opt == 'sgd':
        o = torch.optim.SGD(groups, lr=BASE_LR[opt], momentum=0.9, nesterov=True, weight_decay=WEIGHT_DECAY * decay)
    else:
        o = torch.optim.AdamW(groups, lr=BASE_LR[opt], weight_decay=WEIGHT_DECAY * decay)
    orig = O.drop_path

    def recording(xx, p, training):
        out = orig(xx, p, training)
        if masks is not None and p != 0.0 and training:
            masks.append((out.detach() != 0).flatten(1).any(1))
        return out
    losses = []
    O.drop_path = recording
    try:
        for k in range(steps):
            lr, wd = schedule(opt, k)
            for g in o.param_groups:
                g['lr'] = lr
            o.param_groups[1]['weight_decay'] = wd * decay
            o.zero_grad(set_to_none=True)
            seed_step(k)
            with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
                y = O.timesformer_forward(ps, x.to(dtype), T, heads=HEADS, layers=LAYERS, training=True)
            loss = 0.5 * ((y.to(dtype) - tgt.to(dtype)) ** 2).sum()
            loss.backward()
            with torch.no_grad():
                for p in ps.values():
                    if p.grad is not None and not plain:
                        c = CLIP_GRAD / (p.grad.norm() + 1e-6)
                        if c < 1:
                            p.grad.mul_(c)
            o.step()
            losses.append(loss.item())
    finally:
        O.drop_path = orig
    return {k: v.detach() for k, v in ps.items()}, losses, sd0


def flat(ps, keys=None):
    return torch.cat([ps[k].double().flatten() for k in (keys or sorted(ps))])


def drift(ps, ref, start):
    """||ps - ref|| over ALL parameters, relative to the distance ref travelled from the start."""
    return ((flat(ps) - flat(ref)).norm() / (flat(ref) - flat(start)).norm()).item()


def worst_tensor(ps, ref):
    """(largest relative L2 error of one parameter tensor, its name)."""
    return max((((ps[k].double() - ref[k].double()).norm() / ref[k].double().norm()).item(), k) for k in ref)


def worst_own_travel(ps, ref, start):
    """(largest error of one parameter tensor relative to the distance that tensor travelled, its name)."""
    return max((((ps[k].double() - ref[k].double()).norm() / (ref[k].double() - start[k].double()).norm()).item(), k) for k in ref)
