"""The float64 model of the training tail (csrc/train.hip; tap_net_amd.trainer) and the inputs its tests share: the
formulas of the issue written out in numpy, torch's own float32 form of the same step (``clip_grad_norm_`` + non-fused
``torch.optim.Adam``) whose error against the model is the e_ref of ``pointer_model.tolerance``, and the tensor sets of the
clip-and-Adam cases."""
import numpy as np
import torch

BETAS, EPS = (0.9, 0.999), 1e-8


def losses_model(reward, est, logp):
    """trainer.py:216-225 in float64 with the flagged rule -> adv (B,), seed_logp (B, n), seed_est (B,), stats (5,)"""
    reward, est, logp = (np.asarray(a, np.float64) for a in (reward, est, logp))
    B, n = logp.shape
    ok = np.isfinite(reward)
    adv = np.where(ok, np.where(ok, reward, 0.0) - est, 0.0)
    seed_logp = np.repeat((adv / B)[:, None], n, axis=1)
    seed_est = -2.0 * adv / B
    stats = np.array([(adv * logp.sum(1)).sum() / B, (adv * adv).sum() / B, reward[ok].sum() / B, est[ok].sum() / B, float((~ok).sum())])
    return adv, seed_logp, seed_est, stats


def reference_lines(reward, est, logp):
    """the reference's three lines (trainer.py:216, 222, 225) on torch tensors -> (actor_loss, critic_loss)"""
    advantage = reward - est
    actor_loss = torch.mean(advantage.detach() * logp.sum(dim=1))
    critic_loss = torch.mean(advantage ** 2)
    return actor_loss, critic_loss


def adam_model(p, g, m, v, t, lr, max_norm, betas=BETAS, eps=EPS):
    """one group's step in float64: lists of arrays p, g, m, v, the counter t BEFORE the step -> (p, m, v, norm); a norm that
    is not finite returns the inputs"""
    f = lambda xs: [np.asarray(x, np.float64) for x in xs]                    # noqa: E731
    p, g, m, v = f(p), f(g), f(m), f(v)
    norm = float(np.sqrt(sum(float((x * x).sum()) for x in g)))
    if not np.isfinite(norm):
        return p, m, v, norm
    coef = min(1.0, max_norm / (norm + 1e-6))
    b1, b2 = betas
    t = t + 1
    gc = [x * coef for x in g]
    m = [b1 * a + (1 - b1) * x for a, x in zip(m, gc)]
    v = [b2 * a + (1 - b2) * x * x for a, x in zip(v, gc)]
    p = [a - lr / (1 - b1 ** t) * (mm / (np.sqrt(vv) / np.sqrt(1 - b2 ** t) + eps)) for a, mm, vv in zip(p, m, v)]
    return p, m, v, norm


def adam_torch(p, g, m, v, t, lr, max_norm, dtype=torch.float32, betas=BETAS, eps=EPS):
    """the same step by ``clip_grad_norm_`` + non-fused ``torch.optim.Adam`` on CPU tensors of ``dtype`` -> (p, m, v, norm) as
    float64 arrays"""
    params = [torch.nn.Parameter(torch.tensor(np.asarray(x), dtype=dtype)) for x in p]
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, foreach=False, fused=False)
    for q, gg, mm, vv in zip(params, g, m, v):
        q.grad = torch.tensor(np.asarray(gg), dtype=dtype)
        opt.state[q] = {"step": torch.tensor(float(t)), "exp_avg": torch.tensor(np.asarray(mm), dtype=dtype),
                        "exp_avg_sq": torch.tensor(np.asarray(vv), dtype=dtype)}
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    d = lambda x: x.detach().double().numpy()                                 # noqa: E731
    return [d(q) for q in params], [d(opt.state[q]["exp_avg"]) for q in params], [d(opt.state[q]["exp_avg_sq"]) for q in params], float(norm)


def tail_sizes(chunk):
    """the tensor sizes of the clip-and-Adam cases for a forced ``chunk``; 70 000 gives more than 1 024 partials at chunk 64"""
    return [1, 3, 63, 64, 65, 255, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 70000]


def tail_case(chunk, t, seed):
    """Inputs of one clip-and-Adam case: two groups (the sizes dealt alternately), group 0 clipped (max_norm below its norm),
    group 1 not.  t = 0 (the first step): zero moments and |g| in [1e-3, 1]; t > 0: |g| in [1e-3, 1], exp_avg in [-1, 1] and
    exp_avg_sq in [1e-4, 1] -- inputs on which the update is a smooth function of g.  -> a list of two dicts with float32
    arrays p, g, m, v and lr, max_norm, t."""
    rng = np.random.RandomState(seed)
    sizes = tail_sizes(chunk)
    groups = []
    for gi in range(2):
        mine = sizes[gi::2]
        mag = lambda k: (rng.uniform(1e-3, 1.0, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32)   # noqa: E731
        g = [mag(k) for k in mine]
        p = [rng.uniform(-1, 1, k).astype(np.float32) for k in mine]
        if t == 0:
            m, v = [np.zeros(k, np.float32) for k in mine], [np.zeros(k, np.float32) for k in mine]
        else:
            m = [rng.uniform(-1, 1, k).astype(np.float32) for k in mine]
            v = [rng.uniform(1e-4, 1.0, k).astype(np.float32) for k in mine]
        norm = float(np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in g)))
        groups.append(dict(p=p, g=g, m=m, v=v, t=t, lr=(1e-3, 5e-4)[gi], max_norm=(0.25 * norm, 4.0 * norm)[gi]))
    return groups
