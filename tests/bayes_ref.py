"""fp64 reference of the BAYESIAN arch (networks.py:194-204, policy_v_network.py:80-81), built from
the oracle's NIPS pieces plus numpy for tf.nn.dropout and fc4 (not a test module).

    H3 = act(flat @ W3 + b3)                       the NIPS trunk + fc3
    D  = (H3 / keep) * mask                        tf.nn.dropout; keep == 1: D = H3
    H4 = act(D @ W4 + b4)                          Network_1/fc4
    heads on H4

The mask is an input (the device's own bytes, or mt_dropout_mask_host's). The TensorFlow facts — the
dropout formula, the Network_1 scope name — are TF 1.x's published behaviour, unpinned by any
checkpoint. The backward follows given activation branches (parity_util.device_branches' idea): at
the gradient's discontinuities fp32 rounding may take either side, and the device's side is followed
after it has been checked away from zero (branches_checked).
"""
import numpy as np

from oracle import nets

W4 = 'Network_1/fc4/fc4_weights'
B4 = 'Network_1/fc4/fc4_biases'
W3 = 'Network/fc3/fc3_weights'
B3 = 'Network/fc3/fc3_biases'


def spec(depth, A, R):
    """The NIPS spec with fc4 inserted after fc3 (TF creation order)."""
    s = nets.arch_spec('NIPS', depth, A, R)
    v = list(s['vars'])
    i = [n for n, _, _ in v].index(B3) + 1
    v[i:i] = [(W4, (256, 256), 1.0 / 16), (B4, (256,), 1.0 / 16)]
    s = dict(s)
    s['vars'] = v
    return s


def np_mix64(z):
    z = np.uint64(z)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def np_mask(seed, row, counter, keep):
    """numpy restatement of the mask formula of include/manette_hip.h: [256] uint8."""
    keep = np.float32(keep)
    if keep == np.float32(1.0):
        return np.ones(256, np.uint8)
    with np.errstate(over='ignore'):
        inner = np_mix64((np.uint64(row) << np.uint64(40)) ^ np.uint64(counter))
        base = np_mix64(np.uint64(seed) ^ inner ^ np.uint64(0xD6E8FEB86659FD93))
        q = np.arange(1, 65, dtype=np.uint64)
        h = np_mix64(base + q * np.uint64(0x9e3779b97f4a7c15))
    fields = np.stack([(h >> np.uint64(16 * k)) & np.uint64(0xffff) for k in range(4)], axis=1).reshape(-1)
    u = fields.astype(np.float32) * np.float32(2.0 ** -16)
    return ((keep + u).astype(np.float32) >= np.float32(1.0)).astype(np.uint8)


def forward(P, obs, mask, keep, depth, A, R, act='relu', alpha=0.1, temp=1.0, dtype=np.float64):
    """(v, pi, rep, cache) under `mask` [B, 256] (ignored at keep == 1)."""
    s = nets.arch_spec('NIPS', depth, A, R)
    flat, layers = nets.trunk_forward(s, P, obs, act, alpha, dtype)
    z3 = flat @ P[W3].astype(dtype) + P[B3].astype(dtype)
    H3 = nets.act_fwd(z3, act, alpha)
    m = np.ones_like(H3) if keep == 1 else np.asarray(mask, dtype)
    D = H3 if keep == 1 else (H3 / dtype(keep)) * m
    z4 = D @ P[W4].astype(dtype) + P[B4].astype(dtype)
    H4 = nets.act_fwd(z4, act, alpha)
    heads = {k: P[k] for k in P if k.startswith('Training/')}
    Wc, bc = (heads['Training/Critic/critic_output/critic_output_%s' % k].astype(dtype) for k in ('weights', 'biases'))
    Wa, ba = (heads['Training/Actor/actor_output/actor_output_%s' % k].astype(dtype) for k in ('weights', 'biases'))
    Wr, br = (heads['Training/Repetition/repetition_output/repetition_output_%s' % k].astype(dtype)
              for k in ('weights', 'biases'))
    v = (H4 @ Wc + bc).reshape(-1)
    pi = nets.softmax((H4 @ Wa + ba) / dtype(temp))
    rep = nets.softmax((H4 @ Wr + br) / dtype(temp))
    cache = dict(spec=s, flat=flat, layers=layers, z3=z3, H3=H3, m=m, D=D, z4=z4, H4=H4, keep=keep)
    return v, pi, rep, cache


def branches_checked(cache, dev, act='relu', near=2e-5):
    """The device's activation branches of conv1, conv2, H3 and H4 (dev = forward_branches), each
    checked against the fp64 pre-activation wherever that is >= near x its RMS away from zero, and
    followed closer than that. Returns dict(branches={conv: bool}, h3=bool, h4=bool, near=count)."""
    pos = (lambda x: x > 0) if act == 'relu' else (lambda x: x >= 0)
    out, nears = {}, 0

    def follow(name, z, y_dev):
        nonlocal nears
        far = np.abs(z) >= near * np.sqrt(np.mean(z * z))
        bad = int(((pos(y_dev) != pos(z)) & far).sum())
        assert bad == 0, (name, bad, 'device activation branch differs from the reference away from 0')
        nears += int((~far).sum())
        return np.where(far, pos(z), pos(y_dev))

    br = {L['name']: follow(L['name'], L['z'], dev[L['name']][0][:len(L['z'])]) for L in cache['layers']}
    n = len(cache['z3'])
    return dict(branches=br, h3=follow('H3', cache['z3'], dev['H3'][:n]), h4=follow('H4', cache['z4'], dev['H'][:n]),
                near=nears)


def loss_and_grads(P, cache, v, pi, rep, a_idx, r_idx, y, adv, beta, act='relu', alpha=0.1, temp=1.0,
                   dtype=np.float64, br=None):
    """Loss of policy_v_network.py:25-74 at the train step's own (v, pi, rep) — the outputs under the
    train step's mask — with `adv` fed in (y - the ROLLOUT's values), and the gradient of every
    variable. br = branches_checked(...) or None (the reference's own branches)."""
    s = cache['spec']
    # the head maths of the oracle, on H4 with fc4 as "the dense layer" whose input is D
    s4 = dict(s)
    s4['fc'] = ('fc4', 256)
    P4 = dict(P)
    P4['Network/fc4/fc4_weights'] = P[W4]
    P4['Network/fc4/fc4_biases'] = P[B4]
    c = dict(h=cache['H4'], fc_in=cache['D'])
    loss, G, dD, aux = nets.heads_loss_and_grads(s4, P4, v, pi, rep, c, a_idx, r_idx, y, adv, beta, act, alpha, temp,
                                                 dtype, None if br is None else br['h4'])
    G[W4] = G.pop('Network/fc4/fc4_weights')
    G[B4] = G.pop('Network/fc4/fc4_biases')
    # tf.nn.dropout's gradient: (g * binary) / keep; then fc3's activation
    dH3 = dD if cache['keep'] == 1 else (dD * cache['m']) / dtype(cache['keep'])
    f3 = nets.act_bwd(cache['H3'], act, alpha) if br is None else nets.branch_factor(br['h3'], act, alpha, dtype)
    dz3 = dH3 * f3
    G[W3] = cache['flat'].T @ dz3
    G[B3] = dz3.sum(0)
    dflat = dz3 @ P[W3].astype(dtype).T
    nets.trunk_backward(s, P, cache['layers'], dflat, G, act, alpha, dtype, None, None if br is None else br['branches'])
    return loss, G, aux
