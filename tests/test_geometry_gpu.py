"""Rollout, learn step, packed learn step and deploy forward on the MI355X at the model geometries of
geometry_cases.py — head counts and widths other than 4 x 16, state sizes other than 8, action counts other
than 4 — against the oracle, with the comparators and bounds of test_gpu_parity (compare_rollout: states,
discrete actions, rewards, terminations bit-exact, log-probs and critic logits within 1e-4; _learn_parity:
loss at 1e-4 relative, every gradient tensor at 1e-4 of its own scale; _fused_vs_autograd; the packed-vs-padded
body).  test_geometry_cpu.py settles each case's inputs without a GPU.

Which test first reaches which kernel instantiation (test ids of this file unless another file is named):

decode (csrc/decode.hip)
  k_attn_decode<32, 0> / <64, 0> (no fused out-projection)   test_rollout_matches_oracle[h2x32-multi] / [h1x64-multi],
                                                             also [h4x32_d320-multi], [h8x64_d512-multi], [cont_a6-multi]
  k_attn_decode<16, 0> (H > 8: attn_fused false at dh = 16)  test_rollout_matches_oracle[h16x16-multi]
  k_attn_decode<16, 1> with H = 3, d = 192                   test_rollout_matches_oracle[h3x16_d192-multi]
  k_decode_row<32> / <64> (the shuffle form of the new key's
    score, the alternative of the DH == 16 DPP row sum)      test_rollout_matches_oracle[h2x32-rows] / [h1x64-rows], [cont_a1-rows] / [cont_a6-rows]
  k_decode_row<16> with two heads per wave (H = 16)          test_rollout_matches_oracle[h16x16-rows]
  k_attn_decode<32|64, 0, true>, k_decode_row<32|64, ., true> test_attn_sink_gpu.py::test_sink_rollout_and_learn_match_oracle[h4x32_gqa2_mem3+zero-*] /
                                                             [h2x64_kv1_zero-*]
  k_attn_decode<16, 2, true> (d = 384: the out-projection
    fused with FJ = 2, with sinks)                           test_attn_sink_gpu.py::test_sink_fused_out_projection_rollout[384]
  k_attn_decode<16, 2, true, true> (the same with ALiBi)     test_attn_alibi_gpu.py::test_alibi_fused_out_projection_rollout[384]
  k_embed<3> (d = 192)                                      test_rollout_matches_oracle[h3x16_d192-multi]
  k_embed<8> with d = 320 (columns past d in the last group) test_rollout_matches_oracle[h4x32_d320-multi]
  k_embed<8> with d = 512                                    test_rollout_matches_oracle[h8x64_d512-multi]
  action embeddings read from memory (A > EMB_AREG = 8)      test_rollout_matches_oracle[h3x16_d192-multi] (A = 9), [h8x16_max-multi] (A = 32);
                                                             (d > 256) [h4x32_d320-multi], [h8x64_d512-multi]
  the staged LDS transpose of the state weights at S != 8    S = 3 [h2x32-multi], 1 [h1x64-multi], 13 [h3x16_d192-multi], 5 [cont_a1-multi];
                                                             unstaged (2 d S > 8192) S = 32 [h8x16_max-multi]; S = 40 test_state_dim_past_the_learn_limit_raises
  k_heads_sample<1> (4 d < 768) with A != 4                  every test_rollout_matches_oracle[*-multi] case with d <= 128 but h16x16
  k_heads_sample<2> (4 d >= 768: K split in two, 32 actor
    columns per workgroup) with A != 4                       [h3x16_d192-multi] (A = 9), [h4x32_d320-multi] (6), [a32_d256-multi] (32: the columns filled exactly)
  k_sample behind the projection GEMM (more than 32 actor
    outputs at 4 d >= 768: continuous A > 16)                test_rollout_matches_oracle[cont_a32_d192-multi] (2 A = 64, its LDS row's whole width)
deploy (Agent.forward, E = 1)                                test_deploy_forward_matches_oracle_cached_decode[h8x64_d512] / [h3x16_d192]

learn (csrc/train.hip)
  k_embed_ln<0> (S != 8, layer 0's norm folded in: d <= 256
    and every layer's n_qkv a multiple of 4)                 test_learn_matches_oracle[h3x16_d192-p0] (S = 13), [h8x16_max-p0] (S = 32 = EMB_MAXS)
  k_embed<0> (S != 8) and the separate LayerNorm launches
    (H = 1 or 2 with the learned mix: n_qkv = .. + Hkv is no
    multiple of 4, so ln_fusable is false)                   test_learn_matches_oracle[h2x32-p0] (S = 3), [h1x64-p0] (S = 1), [cont_a1-p0] / [cont_a6-p0] (S = 5)
  k_embed<8> at d > 256 (two columns per thread)             test_learn_matches_oracle[h4x32_d320-p0], [h8x64_d512-p0]
  k_embed_grad_part<8> (A in 5..8)                           test_learn_matches_oracle[h1x64-p0] (A = 5), [h4x32_d320-p0] (A = 6);
                                                             in xtrl_fractal_train_backward: test_fractal_fused_step_matches_autograd
  k_embed_grad_part<EMB_MAXA> (A > 8)                        test_learn_matches_oracle[h3x16_d192-p0] (A = 9), [h8x16_max-p0] (A = 32)
  k_qkv_prep / k_qkv_prep_bwd, rot_dim 16 / 32               test_learn_matches_oracle[h2x32-p0] / [h1x64-p0]
  H dh other than 64                                         128 [h8x16_max], 48 [h3x16_d192], 256 [h16x16], 512 [h8x64_d512]
  LayerNorm kernels at d = 512 (kMaxDPerLane)                test_learn_matches_oracle[h8x64_d512-p0]
  attention dropout at dh = 32 / 64 in the learn step        test_learn_matches_oracle[h2x32-p0.25] / [h1x64-p0.25]
  n > 128 backward at dh != 16 (no xtrl_attn_bwd_part)       test_fused_step_matches_autograd[h2x32-130]
  packed learn step at dh = 64 / at H dh = 48, d = 192       test_packed_learn_matches_padded_step[h1x64] / [h3x16_d192]
  xtrl_attn_fwd_tokens at dh = 32, ld = 3 H dh = 192         test_fractal_fused_step_matches_autograd
  the learn step's sink kernels at dh = 32 / 64              test_attn_sink_gpu.py (the two configurations above)

attention (csrc/attn.hip), kernel level: test_gpu_parity.py::test_attention_fwd_bwd[2-2-130-32] .. [1-2-200-64]
(more than two key tiles at dh = 32 / 64) and test_attention_dropout_dh32_64_against_host_keep_bits;
k_attn_dead_fwd<64, true> / k_attn_dead_bwd<64, true> (padded rows past the band at dh = 64 with Hkv < H):
test_attn_gqa_gpu.py::test_gqa_forward_and_backward_against_fp64[1-4-2-70-64-7]; the bidirectional path of k_attn_fwd
and the fractal forward's other kernels, one at a time: the table of test_fractal_kernels_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import ref_port as R

import geometry_cases as GC
import test_gpu_parity as G
from test_gpu_parity import tol

pytestmark = pytest.mark.gpu


def _explain_action_mismatch(learner, env, oracle, traj, lens, episodes):
    """A bit-exact action differs: print, for the first differing (slot, step), the oracle's logit row, its
    CDF and the uniform draw — a draw within 1e-5 of a CDF boundary is a tie (the case then takes another seed,
    recorded in geometry_cases.py); anything else is a kernel bug — and the device's logit row of that step
    (from a rollout cut at that step, which leaves the step's logits in the engine)."""
    lens_c = lens.cpu().numpy()
    for i, ep in enumerate(episodes):
        n = min(int(lens_c[i]), ep['len'])
        dev = traj['actions'][i, :n].cpu().numpy()
        ref = np.array([int(m[1]) for m in ep['mem'][:n]])
        if (dev != ref).any() or lens_c[i] != ep['len']:
            break
    else:
        return
    t = int(np.nonzero(dev != ref)[0][0]) if (dev != ref).any() else n - 1
    c = oracle.c
    model = oracle.ema.ema_model
    model.eval()
    episode, gene = oracle.episode_genes[i]
    sim = R.SynthSim(c.seed, 0, episode, c.state_dim, c.num_actions, c.sim_mode, c.hazard_log2)
    state, prev_action, prev_reward = torch.from_numpy(sim.reset()).float(), torch.tensor(-1), torch.tensor(0.)
    latent = oracle.latent(torch.tensor([gene])) if c.evolutionary else None
    cache = None
    with torch.no_grad():
        for step in range(t + 1):
            swr = oracle.rsnorm.apply(torch.cat((state, prev_reward[None])))
            raw, _, _, _, cache = model(swr[:-1].reshape(1, 1, -1), actions=prev_action.reshape(1, 1),
                                        rewards=swr[-1], latent_gene=latent, cache=cache)
            raw = raw.reshape(-1)
            u = float(R.philox_uniform(c.seed, 0, i, step, R.FIELD_SAMPLE, 1)[0])
            action = R.discrete_sample_icdf(raw, torch.tensor(u))
            nxt, reward, _ = sim.step(action.numpy())
            prev_action, prev_reward, state = action, torch.tensor(float(reward)), torch.from_numpy(nxt).float()
    cdf = raw.double().softmax(-1).cumsum(-1)[:-1]
    gap = float((cdf - u).abs().min()) if cdf.numel() else float('inf')
    print(f'action mismatch at slot {i} step {t}: device {int(dev[t])}, oracle {int(ref[t])}; uniform draw {u!r}')
    print('  oracle logits:', raw.tolist())
    print('  oracle CDF boundaries:', cdf.tolist(), f'-> nearest boundary {gap:.3e} away:',
          'a TIE (take another seed)' if gap < 1e-5 else 'NOT a tie: a kernel differs')
    try:
        learner._engine = None
        learner.rollout_device(env, 0, t + 1)
        torch.cuda.synchronize()
        eng = learner._engine_for(env, t + 1)
        live = eng.live_rows[t & 1, :int(eng.live_count[t & 1])].cpu().tolist()
        print('  device logits:', eng.logits[live.index(i)].cpu().tolist())
    except Exception as exc:   # (the diagnosis must not hide the mismatch)
        print('  device logits unavailable:', repr(exc))


def _rollout(c, monkeypatch, path=None, **extra):
    """The device rollout of case ``c`` compared with the oracle's; returns (learner, oracle, traj, lens, genes, cum)."""
    if path is not None:
        monkeypatch.setenv('XTRL_DECODE_ROWS', '1' if path == 'rows' else '0')
    learner, env, oracle = G.make_learner(**c.learner_kwargs(), **extra)
    eng = learner._engine_for(env, c.T)
    if path == 'rows':
        assert eng.rows_max > 0
    elif path == 'multi':
        assert eng.rows_max == 0
    traj, lens, genes, cum = learner.rollout_device(env, 0, c.T)
    torch.cuda.synchronize()
    episodes, fitness = oracle.rollout(0)
    GC.action_conditions(c, episodes)
    try:
        G.compare_rollout(traj, lens, episodes, cont=c.cont)
    except AssertionError:
        if not c.cont:
            _explain_action_mismatch(learner, env, oracle, traj, lens, episodes)
        raise
    if c.evo:
        tol(learner.fitness(cum, torch.tensor([g for _, g in learner.episode_genes])), fitness, 1e-5, 1e-5)
    return learner, oracle, traj, lens, genes, cum


ROLLOUTS = [(c, p) for c in GC.CASES + GC.EXTRA for p in c.paths]


@pytest.mark.parametrize('c,path', ROLLOUTS, ids=[f'{c.id}-{p}' for c, p in ROLLOUTS])
def test_rollout_matches_oracle(c, path, monkeypatch):
    """learner.rollout_device against oracle.rollout(0) on each decode path the case lists: states, discrete
    actions, rewards and terminations bit-exact, log-probs and critic logits within 1e-4, EPO fitness within
    1e-5.  Every case listed for the row-resident step has it (rows_max > 0: d <= 128, not GLU, its LDS within
    96 KiB); the wider ones are multi only (RolloutEngine._rows_max: c.dim > 128)."""
    _rollout(c, monkeypatch, path)


LEARNS = [(c, 0.) for c in GC.CASES + GC.EXTRA] + [(GC.BY_ID[i], 0.25) for i in GC.LEARN_DROPOUT]


@pytest.mark.parametrize('c,p', LEARNS, ids=[f'{c.id}-p{p:g}' for c, p in LEARNS])
def test_learn_matches_oracle(c, p, monkeypatch):
    """Two minibatches of the fused learn step (_learn_parity) on the case's own rollout; p = 0.25: attention
    and feed-forward dropout with the oracle applying the host keep masks."""
    learner, oracle, traj, lens, genes, cum = _rollout(c, monkeypatch)
    assert learner.agent.fused_learn
    seen = G._learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2, dropout=p, cont=c.cont)
    assert len(seen) == 2 and seen[0][0] == c.T


@pytest.mark.parametrize('cid,T', GC.FUSED_VS_AUTOGRAD, ids=[f'{i}-{T}' for i, T in GC.FUSED_VS_AUTOGRAD])
def test_fused_step_matches_autograd(cid, T):
    """_fused_vs_autograd at p = 0.25: T = 70 (two key tiles, lengths 36 45 70 2 44 70 4 58), T = 130 (three
    key tiles and, at dh = 32, the n > 128 backward without the folded dQ pass; lengths 108 130 78 2 55 130 4 81)."""
    c = GC.BY_ID[cid]
    lens = G._fused_vs_autograd(c.cont, c.evo, c.gates, 0.25, T, depth=c.depth, episodes=8, batch=4,
                                hazard=5 if T == 70 else 6, dim=c.d, **c.geom())
    assert int(lens.max()) == T and int(lens.min()) < 8


@pytest.mark.parametrize('cid', GC.PACKED)
def test_packed_learn_matches_padded_step(cid):
    """The body of test_gpu_parity.test_packed_learn_matches_padded_step at T = 40 (lengths 8 23 40 7 40 10 40 11)."""
    c = GC.BY_ID[cid]
    G._packed_vs_padded(c.evo, c.gates, 40, c.d, c.cont, None, depth=c.depth, **c.geom())


@pytest.mark.parametrize('cid', ('h4x32_d320_l2', 'h2x32'))
def test_bucketed_backward_equals_plain_backward(cid):
    """xtrl_train_backward with data-parallel gradient buckets (grad_events: the deferred reductions flushed and
    an event recorded on both streams per bucket) gives bitwise the gradient of the plain backward, on the
    two-block backward without the fused LayerNorms (h4x32_d320_l2: d > 256; h2x32: the learned mix's n_qkv is
    no multiple of 4) — the criterion of test_world1_rccl_bucket_allreduce_leaves_gradient_unchanged, without a
    process group.  The backward is run again on the first minibatch's bound inputs (forward activations and
    loss gradients, which it only reads); the control: two plain backwards agree bitwise."""
    import ctypes as C
    c = GC.BY_ID[cid]
    learner, env, _ = G.make_learner(**c.learner_kwargs(), with_oracle=False)
    agent = learner.agent
    traj, lens, genes, cum = learner.rollout_device(env, 0, c.T)
    assert agent.fused_learn
    G._first_minibatch(agent, traj, lens, genes, learner.fitness(cum, genes))
    step = agent.train_step(c.batch, c.T)   # (the step the minibatch ran on, its inputs still bound)

    def backward(grad_events=None):
        agent.flat.grad.zero_()
        step.backward(grad_events=grad_events)
        torch.cuda.synchronize()
        return agent.flat.grad.clone()

    plain = backward()
    assert float(plain.abs().max()) > 0
    assert torch.equal(backward(), plain)
    # 2 (depth + 2) events, created and recorded once (as distributed.BucketAllReduce.__init__)
    events = [torch.cuda.Event() for _ in range(2 * (c.depth + 2))]
    for e in events:
        e.record()
    handles = (C.c_void_p * len(events))(*[e.cuda_event for e in events])
    bucketed = backward(handles)
    assert all(e.query() for e in events)
    assert torch.equal(bucketed, plain)


@pytest.mark.parametrize('cid', GC.DEPLOY)
def test_deploy_forward_matches_oracle_cached_decode(cid):
    """Agent.forward for 6 steps (E = 1, the KV cache threaded through hiddens) against the oracle's cached
    decode, as test_gpu_parity.test_deploy_forward_matches_oracle_cached_decode."""
    c = GC.BY_ID[cid]
    learner, env, oracle = G.make_learner(**c.learner_kwargs())
    G.deploy_parity(learner, oracle, 6, S=c.S)


# ---- the fractal policy body at H = 2, dh = 32, d = 64, S = 3, A = 5, two levels ------------------------------


def test_fractal_rollout_matches_oracle(monkeypatch):
    c = GC.FRACTAL
    _rollout(c, monkeypatch, fractal_levels=c.depth)


def test_fractal_fused_step_matches_autograd():
    """xtrl_fractal_train_forward / backward at dh = 32 (xtrl_attn_fwd_tokens with ld = 3 H dh = 192) and A = 5
    (k_embed_grad_part<8>) against the reference-mode autograd step, p = 0.25, T = 70."""
    c = GC.FRACTAL
    lens = G._fused_vs_autograd(False, False, False, 0.25, 70, depth=c.depth, episodes=8, batch=4, hazard=5, dim=c.d,
                                fractal=c.depth, **c.geom())
    assert int(lens.max()) == 70 and int(lens.min()) < 8


# ---- the state-size limits: the decode takes S < 64, the fused learn step S <= 32 (train.hip EMB_MAXS) ---------


def test_state_dim_past_the_learn_limit_raises(monkeypatch):
    """S = 40: the rollout is supported (and equals the oracle's); the fused learn step refuses the state size
    in xtrl_train_forward's argument check, before any launch — a RuntimeError naming it, never a wrong result:
    no gradient is written and no weight moves.  The reference-mode autograd step (fused_learn False) takes the
    same minibatch and matches the oracle."""
    c = GC.Geometry('s40', 4, 16, 48, 40, 4, 1, True, GC.ROWS_MULTI, 3, 4, 16, 8)
    learner, oracle, traj, lens, genes, cum = _rollout(c, monkeypatch)
    agent = learner.agent
    agent.flat.grad.fill_(7.)
    weights = agent.flat.flat.clone()
    with pytest.raises(RuntimeError, match=r'state_dim 40 > 32'):
        agent.learn(traj, lens, genes, learner.fitness(cum, genes), update=0)
    torch.cuda.synchronize()
    assert bool((agent.flat.grad == 7.).all()) and torch.equal(agent.flat.flat, weights)
    # the reference-mode autograd step has no such limit: it matches the oracle at S = 40
    agent.fused_learn = False
    seen = G._learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 1)
    assert len(seen) == 1
