"""float64 restatement of the reference's LAMB step (utils/optimizer.py:359-499) with the clip of train_temporal.py:228
applied as clip_grad_norm_ does, for the LAMB tests.  Per tensor (lists of numpy arrays, updated in place):

    g  = clip * grad_scale * grad
    m  = b1 m + (1 - b1) g;   v = b2 v + (1 - b2) g^2
    bc = sqrt(1 - b2^t) / (1 - b1^t) if debias else 1
    wn = min(||p||, clamp_value)                      (p before the update)
    r  = m / (sqrt(v) + eps) + wd p
    an = ||r||;  trust = 1 if wn == 0 or an == 0 else wn / an
    p -= s r,   s = lr bc                             (adam)
                s = fp32(lr bc) * fp32(trust) in fp32  (otherwise: the reference multiplies the float lr * bc by its 0-d
                                                        float32 trust-ratio tensor, and that product is the step's scalar)
"""
import numpy as np


class LambState:
    def __init__(self, params):
        self.m = [np.zeros_like(p, dtype=np.float64) for p in params]
        self.v = [np.zeros_like(p, dtype=np.float64) for p in params]
        self.t = 0
        self.weight_norm = self.adam_norm = self.trust_ratio = None


def lamb_step(params, grads, st, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, clamp_value=10.0, adam=False,
              debias=False, max_norm=None, grad_scale=1.0):
    b1, b2 = betas
    g = [grad_scale * np.asarray(x, dtype=np.float64) for x in grads]
    if max_norm is not None:
        total = np.sqrt(sum(float((x * x).sum()) for x in g))
        coef = min(1.0, max_norm / (total + 1e-6))
        g = [coef * x for x in g]
    st.t += 1
    bc = np.sqrt(1.0 - b2 ** st.t) / (1.0 - b1 ** st.t) if debias else 1.0
    wns, ans, trs = [], [], []
    for i, p in enumerate(params):
        st.m[i] = b1 * st.m[i] + (1.0 - b1) * g[i]
        st.v[i] = b2 * st.v[i] + (1.0 - b2) * g[i] * g[i]
        wn = min(float(np.sqrt((p * p).sum())), clamp_value)
        r = st.m[i] / (np.sqrt(st.v[i]) + eps)
        if weight_decay != 0:
            r = r + weight_decay * p
        an = float(np.sqrt((r * r).sum()))
        trust = 1.0 if wn == 0 or an == 0 else wn / an
        s = lr * bc if adam else float(np.float32(lr * bc) * np.float32(trust))
        params[i] = p - s * r
        wns.append(wn)
        ans.append(an)
        trs.append(trust)
    st.weight_norm, st.adam_norm, st.trust_ratio = np.array(wns), np.array(ans), np.array(trs)
    return params


def config(fx, c):
    """the keyword arguments of configuration `c` of g14_lamb"""
    mn = float(fx[f"{c}.max_norm"])
    return dict(lr=float(fx["lr"]), betas=tuple(float(b) for b in fx[f"{c}.betas"]), eps=float(fx["eps"]),
                weight_decay=float(fx[f"{c}.weight_decay"]), clamp_value=float(fx["clamp_value"]),
                adam=bool(fx[f"{c}.adam"]), debias=bool(fx[f"{c}.debias"]), max_norm=mn if mn > 0 else None)
