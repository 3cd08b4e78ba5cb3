"""The LAMB step of include/qatvit.h (qatvit_optim_lamb_moments / qatvit_optim_lamb_apply) restated with torch ops, one tensor at a time.

    g   <- g * coef
    m   <- b1 * m + (1 - b1) * g                       (grad_averaging=False: m <- b1 * m + g)
    v   <- b2 * v + (1 - b2) * g * g
    r    = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd * p
    trust = ||p||_2 / ||r||_2  if (wd != 0 or always_adapt) and ||p|| > 0 and ||r|| > 0, else 1;   trust_clip: min(trust, 1)
    p   <- p - lr * trust * r

`lamb_ref` is the reference: it takes the fp32 (or already double) tensors, evaluates everything in double and returns double p, m, v and the trust
as a python float.  The clip coefficient is an input.  With ``dtype=torch.float32`` the same lines run in fp32 on whatever device the inputs are on:
that is the "stock fp32 torch ops" evaluation whose own error against the double one sets the bar for the kernels (tests/test_gpu_optim_lamb.py)."""
import torch


def lamb_ref(p, g, m, v, *, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, coef=1.0, grad_averaging=True, always_adapt=False,
             trust_clip=False, dtype=torch.float64):
    b1, b2 = betas
    p, g, m, v = (x.detach().to(dtype) for x in (p, g, m, v))
    g = g * coef
    m = b1 * m + ((1 - b1) * g if grad_averaging else g)
    v = b2 * v + (1 - b2) * g * g
    r = (m / (1 - b1 ** step)) / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps) + weight_decay * p
    trust = 1.0
    if weight_decay != 0 or always_adapt:
        pn, rn = p.norm().item(), r.norm().item()
        if pn > 0 and rn > 0:
            trust = pn / rn
            if trust_clip:
                trust = min(trust, 1.0)
    return p - lr * trust * r, m, v, trust
