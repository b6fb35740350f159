"""Plain PyTorch (CPU) reference of the CaRL agent's LayerNorm variants (carla_model.h:44-64 image_encoder
"roach_ln", :113-175 use_layer_norm / use_layer_norm_policy_head): tests/carla_torch_ref.py with
F.layer_norm at the reference's positions and a dtype argument. With every switch off, update()
returns bitwise what carla_torch_ref.update returns in fp32 (test_carla_ln_cpu pins that), which ties it
to the LibTorch golden. Test infrastructure only.

L is a ppo_amd.CarlaLayout2 (include/ppo_carla.h ppo_carla_layout2); names_and_shapes(L) restates
named_parameters() of the module independently of the library's own name table.

condition(): one ReLU whose input rounds to the other side of zero in fp32 moves whole upstream
gradient tensors (a LayerNorm spreads every element's gradient over its row), so parity tests run on
parameters whose pre-ReLU values stay TAU away from zero: in fp64, layer by layer, the LayerNorm bias
of any element that comes within TAU of zero in any row is nudged until none does."""
import numpy as np
import torch
import torch.nn.functional as F

TAU = 1e-4  # well above the largest fp32-vs-fp64 pre-activation difference seen (7e-6)
LN_EPS = 1e-5


def names_and_shapes(L):
    eln, mln, pln = L.arch.encoder_ln, L.arch.mlp_ln, L.arch.policy_ln
    out = [("action_space_high", ()), ("action_space_low", ())]
    step = 3 if eln else 2
    for i in range(6):
        out += [(f"cnn.{step * i}.weight", (L.conv_oc[i], L.conv_ic[i], L.conv_k[i], L.conv_k[i])),
                (f"cnn.{step * i}.bias", (L.conv_oc[i],))]
        if eln:
            shp = (L.conv_oc[i], L.conv_oh[i], L.conv_ow[i])
            out += [(f"cnn.{step * i + 1}.weight", shp), (f"cnn.{step * i + 1}.bias", shp)]

    def mlp(name, ln, dims):
        st = 3 if ln else 2
        for k, (o, i, normed) in enumerate(dims):
            out.extend([(f"{name}.{st * k}.weight", (o, i)), (f"{name}.{st * k}.bias", (o,))])
            if ln and normed:
                out.extend([(f"{name}.{st * k + 1}.weight", (o,)), (f"{name}.{st * k + 1}.bias", (o,))])

    mlp("linear", mln, [(512, 1280, 1), (256, 512, 1)])
    mlp("state_linear", mln, [(256, L.NM, 1), (256, 256, 1)])
    mlp("value_head", mln, [(256, 256 + L.NV, 1), (256, 256, 1), (1, 256, 0)])
    mlp("policy_head", pln, [(256, 256, 1), (256, 256, 1)])
    out += [("dist_mu.0.weight", (L.A, 256)), ("dist_mu.0.bias", (L.A,)),
            ("dist_sigma.0.weight", (L.A, 256)), ("dist_sigma.0.bias", (L.A,))]
    return out


def ln_tensor_indices(L):
    """(index of the LayerNorm weight, index of its bias) per LayerNorm, forward-registration order"""
    # Conv2d weights are 4-D and Linear weights 2-D: a 3-D or 1-D ".weight" is a LayerNorm's
    return [(k, k + 1) for k, (name, shp) in enumerate(names_and_shapes(L))
            if name.endswith(".weight") and len(shp) in (1, 3)]


def init_params(L, CI):
    """carla_inputs.params (weights U(+-sqrt(6 / fan_in)), every other tensor U(+-0.1)) with the LayerNorm
    weights moved to U(0.5, 1.5), so that mistakes in the affine gradients show"""
    p = CI.params(L)
    for gi, _ in ln_tensor_indices(L):
        o, n = L.t_off[gi], L.t_len[gi]
        p[o:o + n] = np.float32(1.0) + np.float32(5.0) * p[o:o + n]
    return p


def _tensors(L, p, dtype):
    ns = names_and_shapes(L)
    assert len(ns) == L.ntensors
    t = {}
    for k, (name, shp) in enumerate(ns):
        o, n = L.t_off[k], L.t_len[k]
        assert n == int(np.prod(shp, dtype=np.int64)), (name, n, shp)
        t[name] = torch.tensor(p[o:o + n].reshape(shp), dtype=dtype, requires_grad=bool(L.t_grad[k]))
    return [n for n, _ in ns], t


def _net(L, t, bev, meas, vmeas, dtype, pre_relu=None):
    """trunk and heads up to (alpha - beta_min, beta - beta_min, value); pre_relu(name, z, u) may return a
    replacement for the normalised pre-ReLU tensor u (condition() uses it)"""
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

    x = torch.tensor(bev).to(dtype) / 255.0
    step = 3 if eln else 2
    for i in range(6):
        x = F.conv2d(x, t[f"cnn.{step * i}.weight"], t[f"cnn.{step * i}.bias"], stride=L.conv_s[i])
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


def _beta_lp_ent(al, be, x):
    ab = al + be
    lp = torch.xlogy(al - 1.0, x) + torch.xlogy(be - 1.0, 1.0 - x) + torch.lgamma(ab) - torch.lgamma(al) - torch.lgamma(be)
    ent = (torch.lgamma(al) + torch.lgamma(be) - torch.lgamma(ab) - (2.0 - ab) * torch.digamma(ab)
           - ((al - 1.0) * torch.digamma(al) + (be - 1.0) * torch.digamma(be)))
    return lp.sum(1), ent.sum(1)


def condition(L, p, bev, meas, vmeas, tau=TAU):
    """Returns (conditioned copy of p, number of nudged bias elements). One fp64 forward: each LayerNorm's
    bias is fixed before the layers after it are computed, so no later layer undoes an earlier one."""
    p = p.copy()
    names, t = _tensors(L, p, torch.float64)
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
            with torch.no_grad():  # 4 tau * k at the k-th try (a step may land beside another row's value)
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
    _, t = _tensors(L, p, torch.float64)
    best = [float("inf")]

    def see(name, z, u):
        best[0] = min(best[0], float(u.abs().min()))

    with torch.no_grad():
        _net(L, t, bev, meas, vmeas, torch.float64, pre_relu=see)
    return best[0]


def forward(L, p, bev, meas, vmeas, act, beta_min=1.0, dtype=torch.float32):
    """AgentImpl::forward with given actions, plus the "mean" action: dict of numpy arrays"""
    _, t = _tensors(L, p, dtype)
    with torch.no_grad():
        mu, sg, value = _net(L, t, bev, meas, vmeas, dtype)
        al, be = F.softplus(mu) + beta_min, F.softplus(sg) + beta_min
        hi, lo = t["action_space_high"], t["action_space_low"]
        a = torch.clamp((torch.tensor(act, dtype=dtype) - lo) / (hi - lo), 1e-7, 1.0 + 1e-7)
        lp, ent = _beta_lp_ent(al, be, a)
        mean = al / (al + be)
        lpm, _ = _beta_lp_ent(al, be, mean)
        out = dict(alpha=al, beta=be, value=value, logprob=lp, entropy=ent, mean_action=mean * (hi - lo) + lo,
                   mean_logprob=lpm)
    return {k: v.numpy() for k, v in out.items()}


def update(L, p, bev, meas, vmeas, act, old_logp, adv, ret, old_v, clip=0.2, ent_coef=0.01, vf_coef=0.5,
           max_grad_norm=0.5, lr=3e-4, eps=1e-5, beta_min=1.0, norm_adv=True, clip_vloss=True, dtype=torch.float32):
    """One PPO minibatch (ac_ppo_carla.cpp:540-619), as carla_torch_ref.update: (grad, stats, total norm,
    stepped parameters, log-prob, value)."""
    names, t = _tensors(L, p, dtype)
    mu, sg, value = _net(L, t, bev, meas, vmeas, dtype)
    al = F.softplus(mu) + beta_min
    be = F.softplus(sg) + beta_min
    hi, lo = t["action_space_high"], t["action_space_low"]
    a = (torch.tensor(act, dtype=dtype) - lo) / (hi - lo)
    a = torch.clamp(a, 1e-7, 1.0 + 1e-7)
    lp, ent = _beta_lp_ent(al, be, a)
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
