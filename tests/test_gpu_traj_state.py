"""The state this library carries from one training step to the next, held to BIT EQUALITY over K = 4 steps of the training stack
(tests/traj.py): the staged W / W^T copies (vtx.functions._wcache) and their in-place restaging through a cached pointer table
(_restage_tables), the merged projection (_mcache), the optimizers' device tables of raw pointers with their lr / wd entries
(vtx.optim._table_cache), the version bumps that tell the weight cache about a kernel's update, the pinned upload slots of the
DropPath scale vectors and FFN compaction tables, the persistent GEMM's counter buffer and the per-call dropout seeds.

Every kernel is deterministic and every random draw comes from the CPU default generator, so a run that keeps all of that state
("warm": no device synchronisation between steps, the host runs ahead as in training) must equal, in every bit of every step's
loss, every parameter and every optimizer state tensor and step count, a run that throws it away at every step ("cold"), a run
resumed from a checkpoint, a run with eval forwards in between, a run with recomputation, a run that shares the process with
another model, and so on.  A difference is a bug in carried state, never rounding: no assertion of the arms has a tolerance.
The negative controls at the end break the Python side of that state on purpose (wrong arithmetic, no fault) and must differ.

The last part holds the same SGD trajectory against oracle/vt_oracle.py in float64."""
import gc

import pytest
import torch

import traj
from helpers import AUTOCAST_FACTOR, TOL_F32, report
from traj import K, Traj, diff, run

pytestmark = pytest.mark.gpu

PRECS = ['bf16', 'fp32']
OPTS = ['sgd', 'adamw']
_ref = {}


def ref(arm='warm', **kw):
    """One trajectory per configuration, computed once and shared (never modified) by the tests that compare with it."""
    key = (arm,) + tuple(sorted(kw.items()))
    if key not in _ref:
        _ref[key] = run(arm, **kw)
    return _ref[key]


def same(a, b, what):
    d = diff(a, b)
    assert not d, f'{what}: the two trajectories differ:\n  ' + '\n  '.join(d[:12])


@pytest.fixture(autouse=True)
def _modes_back():
    import vtx
    yield
    vtx.set_precision('auto')
    vtx.set_stream('bf16')
    vtx.set_recompute(False)


# ------------------------------------------------------------------------------------------------------------------ 1. cold
@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_warm_equals_cold(prec, opt):
    same(ref(prec=prec, opt=opt), ref('cold', prec=prec, opt=opt), f'warm vs cold {prec} {opt}')


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('stream', ['fp32', 'fp32+grad'])
def test_warm_equals_cold_under_the_exact_stream(stream, opt):
    """bf16 kernels with the float32 residual stream.  The exact stream refuses embedding dropout: dropout_p 0 here."""
    kw = dict(prec='bf16', opt=opt, stream=stream, dropout_p=0.0)
    same(ref(**kw), ref('cold', **kw), f'warm vs cold, stream {stream}, {opt}')


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_warm_equals_cold_vivit_fact_encoder(prec, opt):
    kw = dict(prec=prec, opt=opt, model='vivit')
    same(ref(**kw), ref('cold', **kw), f'ViViT fact_encoder warm vs cold {prec} {opt}')


@pytest.mark.parametrize('prec', PRECS)
def test_warm_equals_cold_with_block_dropout(prec):
    """proj_drop and the FFN's dropout_p at 0.1 as well, set by hand (the models' constructors do not take them): one dropout
    seed per sub-block forward.  These masks switch the merged projection and the FFN compaction off (tests/traj.py)."""
    kw = dict(prec=prec, opt='sgd', block_drop=0.1)
    same(ref(**kw), ref('cold', **kw), f'block dropout warm vs cold {prec}')
    assert diff(ref(**kw), ref(prec=prec, opt='sgd')), 'block dropout changed nothing'


# ---------------------------------------------------------------------------------------------------------------- 2. resume
@pytest.mark.parametrize('clear', [False, True])
@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_resume_after_two_steps(prec, opt, clear, tmp_path):
    """torch.save of both state dicts after two steps, everything dropped, new objects with another initialisation,
    load_state_dict from the file.  clear=False: Module.load_state_dict is a versioned copy_, the weight cache notices alone."""
    r = run('warm', prec=prec, opt=opt, resume_at=2, path=str(tmp_path / 'ckpt.pth'), clear=clear)
    same(ref(prec=prec, opt=opt), r, f'warm vs resume-at-2 {prec} {opt} clear={clear}')


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_roll_back_into_the_live_objects(prec, opt, tmp_path):
    """A step is taken and thrown away: both state dicts go back into the LIVE model and optimizer.  The staged copies of the
    discarded weights sit in the cache under the same parameter objects and addresses; only the version counter (copy_) differs."""
    r = run('warm', prec=prec, opt=opt, rollback_at=2, path=str(tmp_path / 'back.pth'))
    same(ref(prec=prec, opt=opt), r, f'roll-back {prec} {opt}')


@pytest.mark.parametrize('opt', OPTS)
def test_buckets_rebuilt_under_a_live_optimizer(opt):
    """New GradBuckets before every step while the optimizer lives on: its cached device tables hold the old gradient addresses."""
    same(ref(prec='bf16', opt=opt), run('warm', prec='bf16', opt=opt, fresh_buckets=True), f'fresh buckets, live optimizer, {opt}')


@pytest.mark.parametrize('opt', OPTS)
def test_optimizer_reloads_its_own_state_in_place(opt):
    """load_state_dict on a LIVE optimizer replaces the state tensors its device tables point at."""
    same(ref(prec='bf16', opt=opt), run('warm', prec='bf16', opt=opt, reload_at=2), f'in-place reload {opt}')


# ------------------------------------------------------------------------------------------------------ 3. eval between steps
@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_eval_forwards_between_steps(prec, opt):
    """After every step an eval forward under no_grad (need_t False on cache entries the next training forward needs with
    W^T; the merged projection's keep scale 1.0 instead of 1 / (1 - p)) and a training forward without backward, while the
    optimizer restages in place.  The trajectory does not move, and every eval output is that of a cold model with those weights."""
    t = Traj(prec=prec, opt=opt, evals=True)
    try:
        for k in range(K):
            t.step(k)
        r = t.result()
        cold = [traj.cold_eval(w, t.xh, **t.kind) for w in t.eval_weights]
    finally:
        t.close()
    same(ref(prec=prec, opt=opt), r, f'eval between steps {prec} {opt}')
    for k in range(K):
        assert torch.equal(r['evals'][k], cold[k]), f'{prec} {opt}: eval output after step {k} is not the cold model\'s'
    assert not torch.equal(r['evals'][0], r['evals'][K - 1])


# ------------------------------------------------------------------------------------------------------------- 4. recompute
@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_recompute_equals_stored_activations(prec, opt):
    same(ref(prec=prec, opt=opt), run('warm', prec=prec, opt=opt, recompute=True), f'recompute {prec} {opt}')


@pytest.mark.parametrize('prec', PRECS)
def test_recompute_equals_stored_activations_with_block_dropout(prec):
    kw = dict(prec=prec, opt='sgd', block_drop=0.1)
    same(ref(**kw), run('warm', recompute=True, **kw), f'recompute with block dropout {prec}')


# ------------------------------------------------------------------------------------------------ 5. two models, one process
@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_two_models_step_alternately(prec, opt):
    solo_a, solo_b = ref(prec=prec, opt=opt), ref(prec=prec, opt=opt, D=64)
    a, b = Traj(prec=prec, opt=opt), Traj(prec=prec, opt=opt, D=64)
    try:
        for k in range(K):
            a.step(k)
            b.step(k)
        ra, rb = a.result(), b.result()
    finally:
        a.close()
        b.close()
    same(solo_a, ra, f'model A beside model B {prec} {opt}')
    same(solo_b, rb, f'model B beside model A {prec} {opt}')


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_model_built_where_another_one_died(prec, opt):
    """A model takes a step and is deleted; its successor, with other weights, very likely gets the same allocations and id()s."""
    solo = ref(prec=prec, opt=opt)
    a = Traj(prec=prec, opt=opt, seed=traj.MODEL_SEED + 3)
    try:
        a.step(0)
        torch.cuda.synchronize()
    finally:
        a.drop()
    del a
    gc.collect()
    same(solo, run('warm', prec=prec, opt=opt), f'successor model {prec} {opt}')


# --------------------------------------------------------------------------------------------------- 6. precision alternating
@pytest.mark.parametrize('opt', OPTS)
def test_precision_alternates_between_steps(opt):
    """bf16, fp32, bf16, fp32 on one model: each dtype's cache entry lives through an update made in the other dtype."""
    kw = dict(opt=opt, precs=('bf16', 'fp32'))
    same(ref(**kw), ref('cold', **kw), f'alternating precision warm vs cold {opt}')
    assert diff(ref(**kw), ref(prec='bf16', opt=opt))
    # with forwards between the steps: the next step's forward, in the OTHER dtype, meets the entries those forwards left
    # behind with the weights unchanged in between
    same(ref(**kw), run('warm', evals=True, **kw), f'alternating precision with forwards in between {opt}')


# -------------------------------------------------------------------------------------------------------------- 7. late joiner
@pytest.mark.parametrize('prec', PRECS)
def test_late_joiner_adamw(prec, tmp_path):
    """Layer 0's temporal attention sub-block (temporal_fc among its parameters) is outside the graph for two steps and joins
    then: buckets.unfired() -> set_skipped keeps it without update, AdamW's bias correction runs on its OWN step count."""
    kw = dict(prec=prec, opt='adamw', late=True)
    w = ref(**kw)
    same(w, ref('cold', **kw), f'late joiner warm vs cold {prec}')
    same(w, run('warm', resume_at=traj.LATE_UNTIL, path=str(tmp_path / 'late.pth'), **kw), f'late joiner warm vs resume {prec}')
    late = [n for n in w['params'] if n.startswith('transformer_layers.layers.0.attentions.0.')]
    assert len(late) == 8 and any('temporal_fc' in n for n in late)
    assert all(w['steps'][n] == K - traj.LATE_UNTIL for n in late), {n: w['steps'][n] for n in late}
    assert all(s == K for n, s in w['steps'].items() if n not in late)
    start = traj.build_model()[1]
    one = run('warm', steps=traj.LATE_UNTIL, **kw)
    assert all(torch.equal(one['params'][n], start[n]) for n in late), 'a parameter outside the graph moved (decay?)'
    assert all(not torch.equal(w['params'][n], start[n]) for n in late), 'the late joiner never joined'


# ------------------------------------------------------------------------------------------- single parameters; what is carried
@pytest.mark.parametrize('prec', PRECS)
def test_an_update_of_any_single_parameter_is_noticed(prec):
    """Every parameter in turn is changed ALONE through its versioned interface (add_ under no_grad) between two training-mode
    forwards: the forward over the warm caches equals the forward after clear_weight_cache().  An optimizer moves all
    parameters at once; a cache stamp that forgot one of them (the merged projection's four) would pass every trajectory."""
    import vtx
    from vtx import functions
    vtx.set_precision(prec)
    m, _ = traj.build_model()
    x = traj.data()[0].to(traj.DEV)

    def fwd():
        traj.seed_step(1)
        return m(x).detach().clone()
    fwd()
    moved = 0
    for n, p in m.named_parameters():
        before = fwd()                                       # (leaves the caches staged for the weights as they are)
        with torch.no_grad():
            p.add_(0.05 * p.abs().mean() + 0.01)
        warm = fwd()
        functions.clear_weight_cache()
        cold = fwd()
        assert torch.equal(warm, cold), f'{prec}: a change of {n} alone went unnoticed by the caches'
        moved += int(not torch.equal(before, cold))
    assert moved >= len(list(m.parameters())) - 2 * traj.LAYERS * 2      # (a key bias moves no output: softmax is shift-invariant)


@pytest.mark.parametrize('opt', OPTS)
@pytest.mark.parametrize('prec', PRECS)
def test_the_warm_arm_really_carries_its_state(prec, opt, monkeypatch):
    """The other side of the equalities: the warm arm must not be a cold arm in disguise.  After the first step no parameter is
    cast or transposed again by ``weights()`` (the optimizer's restage keeps the staged copies and their stamps valid), the
    restage pointer table is built once, and the optimizer builds its device table once."""
    from vtx import functions, ops, optim
    t = Traj(prec=prec, opt=opt)
    ptrs = {p.data_ptr() for p in t.model.parameters()}
    casts, tables, builds, step = [], [], [], [0]
    o_cast, o_table, o_build = ops.cast_transpose, ops.ct_table, optim._FusedBase._build

    def cast(W, dtype, want_c=True, want_t=True):
        if W.data_ptr() in ptrs and (dtype != torch.float32 or want_t):      # (float32 without W^T is the parameter itself: no launch)
            casts.append(step[0])
        return o_cast(W, dtype, want_c=want_c, want_t=want_t)

    def table(*a, **kw):
        tables.append(step[0])
        return o_table(*a, **kw)

    def build(self, ent):
        builds.append(step[0])
        return o_build(self, ent)
    monkeypatch.setattr(ops, 'cast_transpose', cast)
    monkeypatch.setattr(ops, 'ct_table', table)
    monkeypatch.setattr(optim._FusedBase, '_build', build)
    functions.clear_weight_cache()
    try:
        for k in range(K):
            step[0] = k
            t.step(k)
        r = t.result()
    finally:
        t.close()
    same(ref(prec=prec, opt=opt), r, 'the instrumented warm run')
    assert casts and set(casts) == {0}, f'weights() staged parameters again in steps {sorted(set(casts))}'
    assert tables == [0], f'restage tables built in steps {tables}'
    assert builds == [0], f'optimizer tables built in steps {builds}'


# ------------------------------------------------------------------------------------------------- the premise, on the device
def test_dropout_seeds_follow_the_cpu_generator():
    """With DropPath switched off by hand only the embedding dropout's seed is drawn: the same torch.manual_seed gives the same
    output, another one another output -- a resumed or recomputed run reproduces the masks, and no two steps share them."""
    import transformer as T_
    import vtx
    vtx.set_precision('bf16')
    m, _ = traj.build_model()
    for mod in m.modules():
        if isinstance(mod, T_.DropPath):
            mod.dropout_p = 0.0
    x = traj.data()[0].to(traj.DEV)
    outs = []
    with torch.no_grad():
        for k in (0, 0, 1):
            traj.seed_step(k)
            outs.append(m(x))
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


def test_the_model_draws_the_predicted_masks_and_compacts(monkeypatch):
    """tests/test_traj_premise.py predicts which clips each step's FFN drops (and that two steps drop SOME clips, differently);
    here the model's own draws are recorded: the dropout seed drawn before the blocks included, they are the predicted ones,
    and the partial drops go through the compaction plan (its table upload re-uses a pinned slot with new contents)."""
    from vtx import functions
    seen, orig = [], functions._compaction_plan

    def recording(scale_vec, n_units, rows_per, device):
        plan = orig(scale_vec, n_units, rows_per, device)
        host = getattr(scale_vec, '_vtx_host', None) if scale_vec is not None else None
        if host is not None:
            seen.append(([bool(v == 0) for v in host.tolist()], rows_per, plan is not None))
        return plan
    monkeypatch.setattr(functions, '_compaction_plan', recording)
    run('warm', prec='bf16', opt='sgd')
    want = [pat[1] for pat in traj.step_patterns()]
    assert [s[0] for s in seen] == want, (seen, want)
    assert all(rows == 1 + traj.P * traj.T and planned == (0 < sum(pat) < traj.B) for pat, rows, planned in seen)
    assert sum(1 for s in seen if s[2]) >= 2


# ----------------------------------------------------------------------------------------------------------- negative controls
def test_control_no_version_bump_is_noticed(monkeypatch):
    from vtx import optim
    cold = ref('cold', prec='bf16', opt='sgd')
    monkeypatch.setattr(optim._FusedBase, '_bump_versions', lambda self: None)
    assert diff(run('warm', prec='bf16', opt='sgd'), cold), 'stale staged weights went unnoticed'


def test_control_stale_lr_and_weight_decay_are_noticed(monkeypatch):
    """The hyper-parameter refresh of _sync_tables skipped after an optimizer's first step."""
    from vtx import optim
    cold = ref('cold', prec='bf16', opt='sgd')
    orig = optim._FusedBase._sync_tables

    def stale(self):
        if getattr(self, '_synced_once', False):
            hyper = tuple((float(g['lr']), float(g['weight_decay'])) for g in self.param_groups)
            for t in self._table_cache.values():
                t.hyper = hyper                              # "already up to date"
        self._synced_once = True
        return orig(self)
    monkeypatch.setattr(optim._FusedBase, '_sync_tables', stale)
    assert diff(run('warm', prec='bf16', opt='sgd'), cold), 'a stale lr / weight decay went unnoticed'


def test_control_tables_kept_across_load_state_dict_are_noticed(monkeypatch):
    """load_state_dict that keeps _table_cache: the tables go on pointing at the replaced state tensors (kept alive here, so the
    kernels write into live memory that nobody reads any more)."""
    from vtx import optim
    cold = ref('cold', prec='bf16', opt='sgd')
    orig = optim._FusedBase.load_state_dict

    def keeps(self, state_dict):
        tables = self._table_cache
        self._replaced = getattr(self, '_replaced', []) + [[v for st in self.state.values() for v in st.values() if torch.is_tensor(v)]]
        orig(self, state_dict)
        self._table_cache = tables
    monkeypatch.setattr(optim._FusedBase, 'load_state_dict', keeps)
    assert diff(run('warm', prec='bf16', opt='sgd', reload_at=2), cold), 'tables of replaced state tensors went unnoticed'


def test_control_lost_step_count_is_noticed(monkeypatch, tmp_path):
    """state_dict() without the per-parameter 'step': the resumed AdamW restarts its bias correction."""
    from vtx import optim
    warm = ref(prec='bf16', opt='adamw')
    orig = optim._FusedBase.state_dict

    def no_step(self):
        sd = orig(self)
        sd['state'] = {i: {key: v for key, v in st.items() if key != 'step'} for i, st in sd['state'].items()}
        return sd
    monkeypatch.setattr(optim._FusedBase, 'state_dict', no_step)
    t = Traj(prec='bf16', opt='adamw')
    try:
        for k in range(2):
            t.step(k)
        t.save(str(tmp_path / 'nostep.pth'))
        losses = t.losses
        t.drop()
        t = Traj.resumed(str(tmp_path / 'nostep.pth'), losses, prec='bf16', opt='adamw')
        for k in range(2, K):
            t.step(k)
        torch.cuda.synchronize()
        got = {n: v.detach().cpu() for n, v in t.model.state_dict().items()}
    finally:
        t.close()
    assert any(not torch.equal(got[n], warm['params'][n]) for n in got), 'a lost step count went unnoticed'


# ------------------------------------------------------------------------------------------------------------ against float64
_oracle = {}


def _oracle_runs():
    if not _oracle:
        _oracle['f64'] = traj.oracle_run(torch.float64)
        _oracle['f32'] = traj.oracle_run(torch.float32)
        _oracle['amp'] = traj.oracle_run(torch.float32, autocast=True)
    return _oracle


@pytest.mark.parametrize('prec', PRECS)
def test_sgd_trajectory_against_the_float64_oracle(prec):
    """The K-step SGD trajectory of the stack (clipping, decay, schedule, DropPath; dropout off: the oracle has none) against
    oracle/vt_oracle.timesformer_forward in float64 with torch.optim.SGD on the CPU.

    SGD only.  AdamW divides by the root of a second moment that is tiny where a gradient is zero up to rounding (the key bias of
    every attention), so float32 against float64 is already ill-conditioned there: the oracle in float32 against itself in
    float64 is off by 3.4e-2 on its worst tensor, 0.35 of that tensor's travel, where SGD gives 9.4e-7 (tests/test_traj_premise.py
    keeps both numbers true).

    fp32: every parameter tensor within TOL_F32 (relative L2); the ratio of the worst tensor to the oracle's own float32 run
    is reported, not asserted.  bf16: the drift of all parameters relative to the distance travelled is at most AUTOCAST_FACTOR
    (2, the factor of the bf16 gradient bars) times the drift of the oracle under torch.autocast('cpu', bfloat16) on the same
    trajectory -- a yardstick measured on the reference arithmetic, never on the code under test."""
    o = _oracle_runs()
    p64, l64, start = o['f64']
    r = ref(prec=prec, opt='sgd', dropout_p=0.0)
    assert sorted(r['params']) == sorted(p64)
    if prec == 'fp32':
        worst, name = traj.worst_tensor(r['params'], p64)
        yard, yname = traj.worst_tensor(o['f32'][0], p64)
        line = (f'traj fp32 vs float64: worst parameter tensor {worst:.3e} ({name}); the oracle in float32 {yard:.3e} ({yname}): '
                f'ratio {worst / yard:.2f}; drift {traj.drift(r["params"], p64, start):.3e} of the distance travelled '
                f'(oracle float32 {traj.drift(o["f32"][0], p64, start):.3e})')
        print(line)
        report(line)
        for n in p64:
            e = ((r['params'][n].double() - p64[n]).norm() / p64[n].norm()).item()
            assert e <= TOL_F32, f'{n}: {e:.3e} > {TOL_F32}'
        assert max(abs(a - b) / abs(b) for a, b in zip(r['losses'].tolist(), l64)) <= TOL_F32
    else:
        d, amp = traj.drift(r['params'], p64, start), traj.drift(o['amp'][0], p64, start)
        line = f'traj bf16 vs float64: drift {d:.3e} of the distance travelled; the oracle under autocast {amp:.3e}: ratio {d / amp:.2f} (bar {AUTOCAST_FACTOR:g})'
        print(line)
        report(line)
        assert d <= AUTOCAST_FACTOR * amp, line
