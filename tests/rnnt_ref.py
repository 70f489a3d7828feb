"""Float64 numpy restatement of the transducer (RNN-T) pieces, the yardstick of oe_rnnt_loss / oe_rnnt_grad, the joint combine and
TransducerHead (semantics in include/openeat_hip.h).  Written from the definition (Graves 2012) as explicit loops over the
lattice: it shares no code, and no formulation, with the kernels (no anti-diagonals, no log2 domain, and the gradient is
posterior-of-arc minus posterior-of-node times softmax, with the node's posterior taken from alpha + beta)."""
import itertools

import numpy as np


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _feasible(V, Tb, Ub, y, blank):
    return Tb > 0 and all(0 <= int(v) < V and int(v) != blank for v in y[:Ub])


def _alpha_beta(lp, Tb, Ub, y, blank):
    """lp (T, U1, V) log-probabilities of one utterance -> alpha, beta (Tb, Ub+1), logp."""
    alpha = np.full((Tb, Ub + 1), -np.inf)
    alpha[0, 0] = 0.0
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                continue
            terms = []
            if t > 0:
                terms.append(alpha[t - 1, u] + lp[t - 1, u, blank])
            if u > 0:
                terms.append(alpha[t, u - 1] + lp[t, u - 1, y[u - 1]])
            alpha[t, u] = np.logaddexp.reduce(terms)
    beta = np.full((Tb, Ub + 1), -np.inf)
    beta[Tb - 1, Ub] = lp[Tb - 1, Ub, blank]
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                continue
            terms = []
            if t + 1 < Tb:
                terms.append(beta[t + 1, u] + lp[t, u, blank])
            if u < Ub:
                terms.append(beta[t, u + 1] + lp[t, u, y[u]])
            beta[t, u] = np.logaddexp.reduce(terms)
    return alpha, beta, alpha[Tb - 1, Ub] + lp[Tb - 1, Ub, blank]


def rnnt_logp(logits, hlens, targets, ulens, blank=0):
    """logits (B, T, U1, V), hlens (B), targets (B, Umax), ulens (B) -> logp (B) float64; -inf for hlens[b] <= 0 and for an
    utterance with a blank or out-of-range target."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, U1, V = logits.shape
    out = np.full(B, -np.inf)
    for b in range(B):
        Tb, Ub = min(int(hlens[b]), T), int(ulens[b])
        y = [int(v) for v in np.asarray(targets)[b][:Ub]] if Ub > 0 else []
        if not (0 <= Ub <= U1 - 1) or not _feasible(V, Tb, Ub, y, blank):
            continue
        out[b] = _alpha_beta(log_softmax(logits[b]), Tb, Ub, y, blank)[2]
    return out


def rnnt_grad(logits, hlens, targets, ulens, blank=0, g=None):
    """d sum_b g[b] logp[b] / d logits (B, T, U1, V) float64, zeros outside each lattice and for an infeasible utterance."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, U1, V = logits.shape
    g = np.ones(B) if g is None else np.asarray(g, dtype=np.float64)
    d = np.zeros_like(logits)
    for b in range(B):
        Tb, Ub = min(int(hlens[b]), T), int(ulens[b])
        y = [int(v) for v in np.asarray(targets)[b][:Ub]] if Ub > 0 else []
        if not (0 <= Ub <= U1 - 1) or not _feasible(V, Tb, Ub, y, blank):
            continue
        lp = log_softmax(logits[b])
        alpha, beta, logp = _alpha_beta(lp, Tb, Ub, y, blank)
        for t in range(Tb):
            for u in range(Ub + 1):
                node = np.exp(alpha[t, u] + beta[t, u] - logp)              # the posterior of passing through (t,u)
                row = -node * np.exp(lp[t, u])
                if t + 1 < Tb:
                    row[blank] += np.exp(alpha[t, u] + lp[t, u, blank] + beta[t + 1, u] - logp)
                elif u == Ub:
                    row[blank] += np.exp(alpha[t, u] + lp[t, u, blank] - logp)
                if u < Ub:
                    row[y[u]] += np.exp(alpha[t, u] + lp[t, u, y[u]] + beta[t, u + 1] - logp)
                d[b, t, u] = g[b] * row
    return d


def brute_force_logp(logits, Tb, y, blank=0):
    """One utterance, every alignment enumerated: the Tb blanks and len(y) labels in every order that ends on a blank."""
    lp = log_softmax(np.asarray(logits, dtype=np.float64))
    Ub = len(y)
    total = []
    for labels_at in itertools.combinations(range(Tb - 1 + Ub), Ub):        # the last move is the blank of frame Tb-1
        t = u = 0
        s = 0.0
        for i in range(Tb - 1 + Ub):
            if i in labels_at:
                s += lp[t, u, y[u]]
                u += 1
            else:
                s += lp[t, u, blank]
                t += 1
        assert (t, u) == (Tb - 1, Ub)
        total.append(s + lp[t, u, blank])
    return np.logaddexp.reduce(total)


# ---------------------------------------------------------------- the joint network ----
def act(name, x):
    if name in (None, "none"):
        return x
    if name == "tanh":
        return np.tanh(x)
    if name == "relu":
        return np.maximum(x, 0)
    if name == "swish":
        return x / (1 + np.exp(-x))
    raise ValueError(name)


def act_grad(name, x):
    if name in (None, "none"):
        return np.ones_like(x)
    if name == "tanh":
        return 1 - np.tanh(x) ** 2
    if name == "relu":
        return (x > 0).astype(x.dtype)
    if name == "swish":
        s = 1 / (1 + np.exp(-x))
        return s * (1 + x * (1 - s))
    raise ValueError(name)


def lattice_mask(B, T, U1, hlens, ulens):
    m = np.zeros((B, T, U1), dtype=bool)
    for b in range(B):
        Tb = T if hlens is None else int(hlens[b])
        Ub = U1 - 1 if ulens is None else int(ulens[b])
        m[b, :max(Tb, 0), :max(Ub + 1, 0)] = True
    return m


def joint_combine(e, p, hlens=None, ulens=None, activation="tanh", dtype=np.float64):
    """z[b,t,u,:] = act(e[b,t,:] + p[b,u,:]), zeros outside the lattice; evaluated in `dtype`."""
    e, p = np.asarray(e, dtype=dtype), np.asarray(p, dtype=dtype)
    B, T, U1 = e.shape[0], e.shape[1], p.shape[1]
    z = act(activation, e[:, :, None, :] + p[:, None, :, :]).astype(dtype)
    return z * lattice_mask(B, T, U1, hlens, ulens)[..., None]


def joint_combine_grad(e, p, dz, hlens=None, ulens=None, activation="tanh", dtype=np.float64):
    """(de, dp): the sums over u and over t of dz * act'(e + p) inside the lattice, accumulated in index order in `dtype`."""
    e, p, dz = np.asarray(e, dtype=dtype), np.asarray(p, dtype=dtype), np.asarray(dz, dtype=dtype)
    B, T, U1 = e.shape[0], e.shape[1], p.shape[1]
    q = (dz * act_grad(activation, e[:, :, None, :] + p[:, None, :, :]).astype(dtype) * lattice_mask(B, T, U1, hlens, ulens)[..., None]).astype(dtype)
    de, dp = np.zeros_like(e), np.zeros_like(p)
    for u in range(U1):
        de += q[:, :, u, :]
    for t in range(T):
        dp += q[:, t, :, :]
    return de, dp


# ---------------------------------------------------------------- the head ----
class Head:
    """TransducerHead's arithmetic in float64 from its state dict (numpy arrays): a stateless predictor (the last `context`
    tokens, blank before the start, embedded, concatenated, projected, activated) and the joint."""

    def __init__(self, sd, blank=0, context=2, activation="tanh"):
        self.w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
        self.blank, self.context, self.activation = blank, context, activation

    def predictor(self, ctx):
        """ctx (..., context) int -> (..., J)"""
        emb = self.w["embed.weight"][np.asarray(ctx)]
        x = emb.reshape(*emb.shape[:-2], -1)
        return act(self.activation, x @ self.w["pred.weight"].T + self.w["pred.bias"])

    def contexts(self, ys, U1):
        """ys (B, Umax) -> (B, U1, context): position u sees y_{u-context+1} .. y_u, blank before the start"""
        ys = np.asarray(ys)
        B = ys.shape[0]
        padded = np.concatenate([np.full((B, self.context), self.blank, dtype=np.int64), ys[:, :U1 - 1].astype(np.int64)], axis=1)
        return np.stack([padded[:, u:u + self.context] for u in range(U1)], axis=1)

    def logits(self, enc, ys, hlens=None, ulens=None):
        enc = np.asarray(enc, dtype=np.float64)
        U1 = np.asarray(ys).shape[1] + 1
        e = enc @ self.w["enc_proj.weight"].T + self.w["enc_proj.bias"]
        p = self.predictor(self.contexts(ys, U1)) @ self.w["pred_proj.weight"].T
        z = joint_combine(e, p, hlens, ulens, self.activation)
        return z @ self.w["out.weight"].T + self.w["out.bias"]

    def loss(self, enc, hlens, ys, ulens):
        lp = rnnt_logp(self.logits(enc, ys, hlens, ulens), hlens, ys, ulens, self.blank)
        ok = np.isfinite(lp)
        return -lp[ok].sum() / len(lp), lp

    def loss_and_grads(self, enc, hlens, ys, ulens):
        """The loss, its gradient with respect to every weight (a dict keyed like the state dict) and to enc: the chain rule
        written out layer by layer from rnnt_grad's d logits."""
        w = self.w
        enc, ys = np.asarray(enc, dtype=np.float64), np.asarray(ys)
        B, U1 = enc.shape[0], ys.shape[1] + 1
        ctx = self.contexts(ys, U1)
        emb = w["embed.weight"][ctx]
        x = emb.reshape(B, U1, -1)
        pre = x @ w["pred.weight"].T + w["pred.bias"]
        h = act(self.activation, pre)
        e = enc @ w["enc_proj.weight"].T + w["enc_proj.bias"]
        p = h @ w["pred_proj.weight"].T
        z = joint_combine(e, p, hlens, ulens, self.activation)
        logits = z @ w["out.weight"].T + w["out.bias"]
        lp = rnnt_logp(logits, hlens, ys, ulens, self.blank)
        ok = np.isfinite(lp)
        loss = -lp[ok].sum() / B
        dlog = rnnt_grad(logits, hlens, ys, ulens, self.blank, g=np.where(ok, -1.0 / B, 0.0))
        g = {"out.weight": np.einsum("btuv,btuj->vj", dlog, z), "out.bias": dlog.sum(axis=(0, 1, 2))}
        de, dp = joint_combine_grad(e, p, dlog @ w["out.weight"], hlens, ulens, self.activation)
        g["enc_proj.weight"], g["enc_proj.bias"] = np.einsum("btj,btd->jd", de, enc), de.sum(axis=(0, 1))
        g["pred_proj.weight"] = np.einsum("buj,buk->jk", dp, h)
        dpre = (dp @ w["pred_proj.weight"]) * act_grad(self.activation, pre)
        g["pred.weight"], g["pred.bias"] = np.einsum("buj,buk->jk", dpre, x), dpre.sum(axis=(0, 1))
        demb = (dpre @ w["pred.weight"]).reshape(emb.shape)
        g["embed.weight"] = np.zeros_like(w["embed.weight"])
        np.add.at(g["embed.weight"], ctx, demb)
        return loss, g, de @ w["enc_proj.weight"], lp

    def greedy(self, enc, hlens, max_symbols_per_frame=3):
        """Time-synchronous greedy search of one batch -> (tokens, frames, margins): per utterance the emitted tokens, the frame
        of each, and the top-1 margin (in log-probability) of every decision taken, blank decisions included."""
        enc = np.asarray(enc, dtype=np.float64)
        e = enc @ self.w["enc_proj.weight"].T + self.w["enc_proj.bias"]
        toks, frames, margins = [], [], []
        for b in range(enc.shape[0]):
            hyp, fr, mg = [], [], []
            for t in range(int(hlens[b])):
                for _ in range(max_symbols_per_frame):
                    ctx = ([self.blank] * self.context + hyp)[-self.context:]
                    p = self.predictor(np.asarray(ctx)) @ self.w["pred_proj.weight"].T
                    z = act(self.activation, e[b, t] + p)
                    lp = log_softmax(z @ self.w["out.weight"].T + self.w["out.bias"])
                    order = np.argsort(-lp, kind="stable")
                    mg.append(float(lp[order[0]] - lp[order[1]]))
                    if int(order[0]) == self.blank:
                        break
                    hyp.append(int(order[0]))
                    fr.append(t)
            toks.append(hyp)
            frames.append(fr)
            margins.append(mg)
        return toks, frames, margins
