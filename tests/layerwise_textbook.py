"""LARS and LAMB one tensor at a time in fp64, straight from their definitions: what the flat-store optimizers are
tested against on the CPU and on the GPU (not a test module)."""
import math

import torch


class Textbook:
    """The definitions, per parameter, in fp64. ``params``: list of tensors, ``decay``: list of bool. After a step,
    ``last_p`` / ``last_x`` hold what the two norms of each trust ratio were taken over (the weights before the update;
    the scaled gradient for LARS, u for LAMB) and ``ratio`` the ratios."""

    def __init__(self, kind, params, decay, lr, wd, max_grad_norm=None, eta=0.001, mu=0.9, betas=(0.9, 0.999),
                 eps=1e-6):
        self.kind, self.decay, self.lr, self.wd, self.clip = kind, decay, lr, wd, max_grad_norm
        self.eta, self.mu, (self.b1, self.b2), self.eps = eta, mu, betas, eps
        self.p = [t.double().clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.t = 0
        self.ratio = [1.0] * len(self.p)
        self.last_p = [None] * len(self.p)
        self.last_x = [None] * len(self.p)

    def step(self, grads, grad_scale=1.0, lr=None, factor=None):
        lr = self.lr if lr is None else lr
        g = [x.double() * grad_scale for x in grads]
        if factor is None and self.clip:
            norm = math.sqrt(sum(float((x * x).sum()) for x in g))
            factor = min(1.0, self.clip / (norm + 1e-6))
        if factor is not None:
            g = [x * factor for x in g]
        self.t += 1
        for i, (p, gi) in enumerate(zip(self.p, g)):
            wd = self.wd if self.decay[i] else 0.0
            pn = float(p.norm())
            self.last_p[i] = p
            if self.kind == "lamb":
                self.m[i] = self.b1 * self.m[i] + (1 - self.b1) * gi
                self.v[i] = self.b2 * self.v[i] + (1 - self.b2) * gi * gi
                u = (self.m[i] / (1 - self.b1 ** self.t)) / ((self.v[i] / (1 - self.b2 ** self.t)).sqrt() + self.eps)
                u = u + wd * p
                un = float(u.norm())
                self.last_x[i] = u
                r = pn / un if (self.decay[i] and pn > 0 and un > 0) else 1.0
                self.p[i] = p - lr * r * u
            else:
                gn = float(gi.norm())
                self.last_x[i] = gi
                r = self.eta * pn / (gn + self.wd * pn) if (self.decay[i] and pn > 0 and gn > 0) else 1.0
                d = r * (gi + wd * p)
                self.m[i] = d if self.t == 1 else self.mu * self.m[i] + d
                self.p[i] = p - lr * self.m[i]
            self.ratio[i] = r
