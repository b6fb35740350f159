"""Plain PyTorch (CPU) reference of the CaRL agent with use_positional_encoding (carla_model.h:38-42,
:222-236): tests/carla_ln_ref.py restated with the network input built as the reference writes it. Test
infrastructure only.

L is a ppo_amd.CarlaLayout2; conv_ic[0] - C == 2 is the switch. With it on, the input of cnn.0 is

    torch.cat([bev (uint8), grid0, grid1], 1)       grid0, grid1 = meshgrid(linspace(-1, 1, IH),
                                                                            linspace(-1, 1, IW), indexing="ij")

whose first operand is the RAW uint8 tensor: the reference computes bev / 255 and then overwrites it with
this concatenation, which promotes the bytes to fp32, so cnn.0 sees 0..255. The grids are fp32 (torch's
default dtype, as torch::linspace's in the reference) whatever dtype the network runs in: an fp64 run
converts those fp32 values. With the switch off, update() returns bitwise what carla_ln_ref.update returns
(test_carla_pos_cpu pins that).

names_and_shapes, the parameter distributions, the Beta log-prob / entropy and the tensor table are
carla_ln_ref's (cnn.0.weight's shape follows conv_ic[0]); the network, condition(), forward() and update()
are restated here."""
import numpy as np
import torch
import torch.nn.functional as F

import carla_ln_ref as LR
from carla_ln_ref import LN_EPS, TAU, init_params, ln_tensor_indices, names_and_shapes  # noqa: F401


def positional(L):
    d = L.conv_ic[0] - L.C
    assert d in (0, 2), d
    return d == 2


def net_input(L, bev, dtype):
    """what cnn.0 reads (carla_model.h:222-236)"""
    b = torch.tensor(bev)
    assert b.dtype == torch.uint8
    if not positional(L):
        return b.to(dtype) / 255.0
    x = torch.linspace(-1.0, 1.0, L.IH)
    y = torch.linspace(-1.0, 1.0, L.IW)
    g0, g1 = torch.meshgrid(x, y, indexing="ij")
    g0 = g0.unsqueeze(0).unsqueeze(0).expand(b.shape[0], -1, -1, -1)
    g1 = g1.unsqueeze(0).unsqueeze(0).expand(b.shape[0], -1, -1, -1)
    cat = torch.cat([b, g0, g1], 1)  # uint8 with float32: float32, 255 -> 255.0
    assert cat.dtype == torch.float32 and cat.shape[1] == L.C + 2
    return cat.to(dtype)


def _net(L, t, bev, meas, vmeas, dtype, pre_relu=None, zero_pos=False):
    """trunk and heads up to (alpha - beta_min, beta - beta_min, value); pre_relu as carla_ln_ref._net's;
    zero_pos: cnn.0's two positional filters zeroed (the tests' "has teeth" check)"""
    eln, mln, pln = L.arch.encoder_ln, L.arch.mlp_ln, L.arch.policy_ln

    def norm(z, name):
        u = F.layer_norm(z, z.shape[1:], t[name + ".weight"], t[name + ".bias"], LN_EPS)
        if pre_relu is not None:
            r = pre_relu(name, z, u)
            if r is not None:
                u = r
        return u

    def mlp(x, name, ln, nlayers, last_plain=False):
        st = 3 if ln else 2
        for k in range(nlayers):
            x = F.linear(x, t[f"{name}.{st * k}.weight"], t[f"{name}.{st * k}.bias"])
            if last_plain and k == nlayers - 1:
                return x
            if ln:
                x = norm(x, f"{name}.{st * k + 1}")
            x = F.relu(x)
        return x

    x = net_input(L, bev, dtype)
    step = 3 if eln else 2
    for i in range(6):
        w = t[f"cnn.{step * i}.weight"]
        if i == 0 and zero_pos:
            w = torch.cat([w[:, :L.C], torch.zeros_like(w[:, L.C:])], 1)
        x = F.conv2d(x, w, t[f"cnn.{step * i}.bias"], stride=L.conv_s[i])
        if eln:
            x = norm(x, f"cnn.{step * i + 1}")
        x = F.relu(x)
    x = torch.flatten(x, 1)
    s = mlp(torch.tensor(meas, dtype=dtype), "state_linear", mln, 2)
    feat = mlp(torch.cat([x, s], 1), "linear", mln, 2)
    value = mlp(torch.cat([feat, torch.tensor(vmeas, dtype=dtype)], 1), "value_head", mln, 3, last_plain=True).view(-1)
    pi = mlp(feat, "policy_head", pln, 2)
    mu = F.linear(pi, t["dist_mu.0.weight"], t["dist_mu.0.bias"])
    sg = F.linear(pi, t["dist_sigma.0.weight"], t["dist_sigma.0.bias"])
    return mu, sg, value


def scale_image_filters(L, p, s):
    """a copy of p with the image-channel part of cnn.0.weight multiplied by s (1 / 255 gives a positional
    agent without LayerNorm activations of the usual size on its un-normalised input)"""
    p = p.copy()
    w = p[L.conv_w[0]:L.conv_w[0] + L.t_len[2]].reshape(L.conv_oc[0], L.conv_ic[0], L.conv_k[0], L.conv_k[0])
    w[:, :L.C] *= np.float32(s)
    return p


def condition(L, p, bev, meas, vmeas, tau=TAU):
    """carla_ln_ref.condition on this network: (conditioned copy of p, number of nudged bias elements)"""
    p = p.copy()
    names, t = LR._tensors(L, p, torch.float64)
    off = {n: L.t_off[k] for k, n in enumerate(names)}
    nudged = 0

    def fix(name, z, u):
        nonlocal nudged
        b = t[name + ".bias"]
        for k in range(1, 64):
            bad = (u.abs() < tau).flatten(1).any(0).view(b.shape)
            if not bad.any():
                return u
            nudged += int(bad.sum())
            with torch.no_grad():
                nb = (b[bad].float() + np.float32(4 * tau * k)).double()
                b[bad] = nb
            u = F.layer_norm(z, z.shape[1:], t[name + ".weight"], b, LN_EPS)
        raise AssertionError(f"conditioning of {name} did not converge")

    with torch.no_grad():
        _net(L, t, bev, meas, vmeas, torch.float64, pre_relu=fix)
    for n in names:
        if n.endswith(".bias"):
            o = off[n]
            p[o:o + t[n].numel()] = t[n].detach().numpy().reshape(-1).astype(np.float32)
    return p, nudged


def min_pre_relu_distance(L, p, bev, meas, vmeas):
    """smallest |pre-ReLU value| over every LayerNorm of the agent, in fp64 (inf without LayerNorm)"""
    _, t = LR._tensors(L, p, torch.float64)
    best = [float("inf")]

    def see(name, z, u):
        best[0] = min(best[0], float(u.abs().min()))

    with torch.no_grad():
        _net(L, t, bev, meas, vmeas, torch.float64, pre_relu=see)
    return best[0]


def forward(L, p, bev, meas, vmeas, act, beta_min=1.0, dtype=torch.float32, zero_pos=False):
    """AgentImpl::forward with given actions, plus the "mean" action: dict of numpy arrays"""
    _, t = LR._tensors(L, p, dtype)
    with torch.no_grad():
        mu, sg, value = _net(L, t, bev, meas, vmeas, dtype, zero_pos=zero_pos)
        al, be = F.softplus(mu) + beta_min, F.softplus(sg) + beta_min
        hi, lo = t["action_space_high"], t["action_space_low"]
        a = torch.clamp((torch.tensor(act, dtype=dtype) - lo) / (hi - lo), 1e-7, 1.0 + 1e-7)
        lp, ent = LR._beta_lp_ent(al, be, a)
        mean = al / (al + be)
        lpm, _ = LR._beta_lp_ent(al, be, mean)
        out = dict(alpha=al, beta=be, value=value, logprob=lp, entropy=ent, mean_action=mean * (hi - lo) + lo,
                   mean_logprob=lpm)
    return {k: v.numpy() for k, v in out.items()}


def update(L, p, bev, meas, vmeas, act, old_logp, adv, ret, old_v, clip=0.2, ent_coef=0.01, vf_coef=0.5,
           max_grad_norm=0.5, lr=3e-4, eps=1e-5, beta_min=1.0, norm_adv=True, clip_vloss=True, dtype=torch.float32):
    """One PPO minibatch (ac_ppo_carla.cpp:540-619), as carla_ln_ref.update: (grad, stats, total norm,
    stepped parameters, log-prob, value)."""
    names, t = LR._tensors(L, p, dtype)
    mu, sg, value = _net(L, t, bev, meas, vmeas, dtype)
    al = F.softplus(mu) + beta_min
    be = F.softplus(sg) + beta_min
    hi, lo = t["action_space_high"], t["action_space_low"]
    a = (torch.tensor(act, dtype=dtype) - lo) / (hi - lo)
    a = torch.clamp(a, 1e-7, 1.0 + 1e-7)
    lp, ent = LR._beta_lp_ent(al, be, a)
    logratio = lp - torch.tensor(old_logp, dtype=dtype)
    ratio = logratio.exp()
    mb_adv = torch.tensor(adv, dtype=dtype)
    if norm_adv:
        mb_adv = (mb_adv - mb_adv.mean()) / (mb_adv.std() + 1e-8)
    pg = torch.max(-mb_adv * ratio, -mb_adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    R, ov = torch.tensor(ret, dtype=dtype), torch.tensor(old_v, dtype=dtype)
    if clip_vloss:
        vc = ov + torch.clamp(value - ov, -clip, clip)
        vl = 0.5 * torch.max((value - R) ** 2, (vc - R) ** 2).mean()
    else:
        vl = 0.5 * ((value - R) ** 2).mean()
    loss = pg - ent_coef * ent.mean() + vf_coef * vl
    loss.backward()
    with torch.no_grad():
        stats = [pg.item(), vl.item(), ent.mean().item(), (-logratio).mean().item(),
                 ((ratio - 1) - logratio).mean().item(), ((ratio - 1).abs() > clip).float().mean().item()]
    np_dt = np.float32 if dtype == torch.float32 else np.float64
    grad = np.zeros(L.P, np_dt)
    for k, n in enumerate(names):
        if t[n].grad is not None:
            grad[L.t_off[k]:L.t_off[k] + L.t_len[k]] = t[n].grad.numpy().reshape(-1)
    params = [t[n] for n in names]
    total = float(torch.nn.utils.clip_grad_norm_([q for q in params if q.requires_grad], max_grad_norm))
    opt = torch.optim.Adam([q for q in params if q.requires_grad], lr=lr, eps=eps)
    opt.step()
    new_p = np.concatenate([t[n].detach().numpy().reshape(-1) for n in names]).astype(np_dt)
    return grad, np.array(stats, np.float32), total, new_p, lp.detach().numpy(), value.detach().numpy()
