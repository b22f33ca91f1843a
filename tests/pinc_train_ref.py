"""NumPy restatement of the PINc training step (training/train_tank_brov2_full_comparison.py:724-835): PINcNet forward and
backward over all 22 tensors, the three loss terms, clip_grad_norm_ and torch.optim.AdamW.  TEST INFRASTRUCTURE ONLY.

fp64 by default; fp32=True runs every array operation in float32 (the precision the reference and the kernels train in), so that
a test can measure how far fp32 arithmetic itself lands from fp64 on the same inputs -- the yardstick the GPU bounds are multiples
of, as oracle/pinc_numpy.py is for inference.  Pinned against the reference's own autograd by tests/test_pinc_train_cpu.py."""
import numpy as np

from oracle import pinc_numpy

N_IN, N_OUT, HID = 14, 9, 64
LAYERS = (0, 3, 6, 9)
KEYS = tuple(k for i in LAYERS for k in (f"net.{i}.weight", f"net.{i}.bias", f"net.{i + 1}.beta", f"net.{i + 2}.weight", f"net.{i + 2}.bias")) \
    + ("net.12.weight", "net.12.bias")
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, max_norm=5.0)


def shapes():
    s = {}
    for l, i in enumerate(LAYERS):
        s[f"net.{i}.weight"] = (HID, N_IN if l == 0 else HID)
        s[f"net.{i}.bias"] = (HID,)
        s[f"net.{i + 1}.beta"] = ()
        s[f"net.{i + 2}.weight"] = (HID,)
        s[f"net.{i + 2}.bias"] = (HID,)
    s["net.12.weight"] = (N_OUT, HID)
    s["net.12.bias"] = (N_OUT,)
    return s


def flatten(d, dtype=np.float64):
    return np.concatenate([np.asarray(d[k], dtype=dtype).ravel() for k in KEYS])


def unflatten(v):
    out, o = {}, 0
    for k, shp in shapes().items():
        n = int(np.prod(shp, dtype=np.int64))
        out[k] = np.asarray(v[o:o + n]).reshape(shp)
        o += n
    return out


def slices():
    out, o = {}, 0
    for k, shp in shapes().items():
        n = int(np.prod(shp, dtype=np.int64))
        out[k] = slice(o, o + n)
        o += n
    return out


def _cast(sd, f):
    return {k: np.asarray(sd[k], dtype=f) for k in KEYS}


def _forward(p, z, f):
    """-> (x_next [B,9], cache)."""
    h, layers = z, []
    for i in LAYERS:
        W, b, beta, g, be = p[f"net.{i}.weight"], p[f"net.{i}.bias"], p[f"net.{i + 1}.beta"], p[f"net.{i + 2}.weight"], p[f"net.{i + 2}.bias"]
        a = h @ W.T + b
        y = beta * a
        big = y > f(20)
        e = np.exp(np.minimum(y, f(20)))
        sp = np.where(big, y, np.log1p(e))
        sig = np.where(big, f(1), e / (e + f(1)))
        bd = beta + f(1e-12)
        s = sp / bd
        mean = s.mean(axis=1, keepdims=True, dtype=f)
        d = s - mean
        var = (d * d).mean(axis=1, keepdims=True, dtype=f)
        rstd = f(1) / np.sqrt(var + f(1e-5))
        xh = d * rstd
        layers.append((h, a, sp, sig, xh, rstd))
        h = xh * g + be
    dx = h @ p["net.12.weight"].T + p["net.12.bias"]
    c, s = z[:, 3], z[:, 4]
    cb, sb = c + dx[:, 3], s + dx[:, 4]
    r = np.sqrt(cb * cb + sb * sb)
    nrm = np.maximum(r, f(1e-6))
    xn = z[:, :9] + dx
    xn[:, 0] = c * dx[:, 0] - s * dx[:, 1] + z[:, 0]
    xn[:, 1] = s * dx[:, 0] + c * dx[:, 1] + z[:, 1]
    xn[:, 3] = cb / nrm
    xn[:, 4] = sb / nrm
    return xn, (z, layers, h, dx, cb, sb, r, nrm)


def _backward(p, cache, gx, f, grads, terms=None):
    """gx = dL/dx_next [B,9]; adds the parameter gradients to `grads`; returns dL/dz[:, :9].  terms (optional dict): receives, per
    beta key, the list of the elementwise terms [B,64] whose sum is that beta's gradient."""
    z, layers, h4, dx, cb, sb, r, nrm = cache
    c, s = z[:, 3], z[:, 4]
    live = r >= f(1e-6)                                  # torch.clamp passes the gradient where the input is not below the minimum
    dn = np.where(live, -(gx[:, 3] * cb + gx[:, 4] * sb) / (nrm * nrm), f(0))
    rs = np.where(live, r, f(1))
    dcb = gx[:, 3] / nrm + dn * cb / rs
    dsb = gx[:, 4] / nrm + dn * sb / rs
    ddx = gx.copy()
    ddx[:, 0] = gx[:, 0] * c + gx[:, 1] * s
    ddx[:, 1] = gx[:, 1] * c - gx[:, 0] * s
    ddx[:, 3] = dcb
    ddx[:, 4] = dsb
    dz = gx.copy()
    dz[:, 3] = gx[:, 0] * dx[:, 0] + gx[:, 1] * dx[:, 1] + dcb
    dz[:, 4] = gx[:, 1] * dx[:, 0] - gx[:, 0] * dx[:, 1] + dsb
    grads["net.12.weight"] += ddx.T @ h4
    grads["net.12.bias"] += ddx.sum(axis=0, dtype=f)
    dh = ddx @ p["net.12.weight"]
    for l in (3, 2, 1, 0):
        i = LAYERS[l]
        hin, a, sp, sig, xh, rstd = layers[l]
        W, beta, g = p[f"net.{i}.weight"], p[f"net.{i + 1}.beta"], p[f"net.{i + 2}.weight"]
        bd = beta + f(1e-12)
        grads[f"net.{i + 2}.weight"] += (dh * xh).sum(axis=0, dtype=f)
        grads[f"net.{i + 2}.bias"] += dh.sum(axis=0, dtype=f)
        dxh = dh * g
        m1 = dxh.mean(axis=1, keepdims=True, dtype=f)
        m2 = (dxh * xh).mean(axis=1, keepdims=True, dtype=f)
        ds = rstd * (dxh - m1 - xh * m2)
        da = ds * (sig * beta / bd)
        t = ds * ((sig * a - sp / bd) / bd)
        if terms is not None:
            terms.setdefault(f"net.{i + 1}.beta", []).append(t)
        grads[f"net.{i + 1}.beta"] += t.sum(dtype=f)
        grads[f"net.{i}.weight"] += da.T @ hin
        grads[f"net.{i}.bias"] += da.sum(axis=0, dtype=f)
        dh = da @ W
    dz += dh[:, :9]
    return dz


def physics_mean_square(xn, u4, f):
    """physics_loss: mean square of fossen/bluerov_torch.bluerov_compute at the predicted state (fossen/parameters.py)."""
    m, g = 11.4, 9.82
    F_bouy = 1026 * 0.0115 * g
    X_ud, Y_vd, Z_wd, N_rd, I_zz = -2.6, -18.5, -13.3, -0.28, 0.245
    X_u, Y_v, Z_w, N_r = -0.09, -0.26, -0.19, -4.64
    X_uc, Y_vc, Z_wc, N_rc = -34.96, -103.25, -74.23, -0.43
    c, s, u, v, w, r = (xn[:, k] for k in (3, 4, 5, 6, 7, 8))
    X, Y, Z, Mz = (u4[:, k] for k in range(4))
    rhs = np.stack([
        c * u - s * v, s * u + c * v, w, -s * r, c * r,
        f(1 / (m - X_ud)) * (X + f(m - Y_vd) * v * r + (f(X_u) + f(X_uc) * np.abs(u)) * u),
        f(1 / (m - Y_vd)) * (Y - f(m - X_ud) * u * r + (f(Y_v) + f(Y_vc) * np.abs(v)) * v),
        f(1 / (m - Z_wd)) * (Z + (f(Z_w) + f(Z_wc) * np.abs(w)) * w + f(m * g) - f(F_bouy)),
        f(1 / (I_zz - N_rd)) * (Mz - f(X_ud - Y_vd) * u * v + (f(N_r) + f(N_rc) * np.abs(r)) * r)], axis=1)
    return (rhs * rhs).mean(dtype=f)


def loss_and_grad(sd, z, y, u4, K, use_physics=True, fp32=False, terms=None):
    """One minibatch (rows in batch order) -> (loss [3] = (mse, physics mean square, rollout), grads dict, flat gradient in blob
    order).  The gradient is that of loss[0] + loss[2]; the reference's reported loss is loss[0] + 0.5 loss[1] + loss[2].
    terms: see _backward."""
    f = np.float32 if fp32 else np.float64
    p = _cast(sd, f)
    z = np.asarray(z, dtype=f).reshape(-1, N_IN)
    B = z.shape[0]
    y = np.asarray(y, dtype=f).reshape(B, N_OUT)
    grads = {k: np.zeros(np.shape(p[k]), dtype=f) for k in KEYS}
    xn, cache = _forward(p, z, f)
    d = xn - y
    loss = np.zeros(3, dtype=f)
    loss[0] = (d * d).mean(dtype=f)
    _backward(p, cache, d * f(2.0 / (B * N_OUT)), f, grads, terms)
    if use_physics:
        loss[1] = physics_mean_square(xn, np.asarray(u4, dtype=f).reshape(B, 4), f)
    K = int(K)
    if K > 0:
        assert K < B
        caches, x = [], z[0:1, :9]
        for i in range(K):
            zi = np.concatenate([x, z[i:i + 1, 9:13], z[0:1, 13:14]], axis=1)
            x, ch = _forward(p, zi, f)
            caches.append((ch, x))
        carry = np.zeros((1, N_OUT), dtype=f)
        tot = f(0)
        for i in range(K - 1, -1, -1):
            ch, x = caches[i]
            d = x - z[i + 1:i + 2, :9]
            tot = tot + (d * d).mean(dtype=f)
            carry = _backward(p, ch, d * f(2.0 / (N_OUT * K)) + carry, f, grads, terms)
        loss[2] = tot / f(K)
    return loss, grads, flatten(grads, f)


def adamw_step(w, m, v, g, step, lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, max_norm=5.0, fp32=False):
    """clip_grad_norm_(max_norm) then torch.optim.AdamW's step number `step` (1-based) on flat arrays -> (w, m, v, norm)."""
    f = np.float32 if fp32 else np.float64
    w, m, v, g = (np.asarray(a, dtype=f) for a in (w, m, v, g))
    norm = np.sqrt((g * g).sum(dtype=f))
    coef = np.minimum(f(max_norm) / (norm + f(1e-6)), f(1))
    g = g * coef
    w = w * f(1 - lr * weight_decay)
    m = m + (g - m) * f(1 - beta1)
    v = v * f(beta2) + f(1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = np.sqrt(v) / f(np.sqrt(bc2)) + f(eps)
    w = w - f(lr / bc1) * (m / denom)
    return w, m, v, norm


def train(sd, Z, Y, U4, index_lists, rollout_steps=10, use_physics=True, use_rollout=True, fp32=False, state=None, **hyper):
    """The reference's loop body once per index list -> dict(w, m, v (flat), step, losses [iters,3], snap {iteration: (w, m, v)})."""
    f = np.float32 if fp32 else np.float64
    hp = dict(HYPER, **hyper)
    w = flatten(sd, f)
    m, v, step = (np.zeros_like(w), np.zeros_like(w), 0) if state is None else (np.asarray(state[0], f), np.asarray(state[1], f), int(state[2]))
    losses, snap = [], {}
    for idx in index_lists:
        idx = np.asarray(idx)
        B = len(idx)
        K = min(rollout_steps, B - 1) if use_rollout else 0
        loss, _, g = loss_and_grad(unflatten(w), Z[idx], Y[idx], U4[idx], K, use_physics, fp32)
        step += 1
        w, m, v, _ = adamw_step(w, m, v, g, step, fp32=fp32, **hp)
        losses.append(loss)
        snap[step] = (w.copy(), m.copy(), v.copy())
    return dict(w=w, m=m, v=v, step=step, losses=np.array(losses), snap=snap)


def make_dataset(X12, U8, dt, lag=None):
    """make_pinc_dataset with one map vehicle that starts from `lag` -> (z_in, y, U4, lag_after)."""
    X9 = pinc_numpy.to9(X12)
    U4, lag = pinc_numpy.thruster_stream(U8, dt, lag)
    z = np.hstack([X9[:-1], U4[:-1], np.full((len(X9) - 1, 1), float(dt))])
    return z, X9[1:], U4, lag


def beta_conditions(terms64):
    """Condition number |t|_1 / |sum t| of each beta gradient (one number, the sum of 64 terms per row) -> {key: cond}."""
    out = {}
    for k in terms64:
        t = np.concatenate([np.asarray(a, np.float64).ravel() for a in terms64[k]])
        tot = abs(float(t.sum()))
        out[k] = float(np.abs(t).sum()) / tot if tot > 0 else float("inf")
    return out


def tensor_rel_errors(a, b):
    """per-tensor |a - b|_2 / |b|_2 of two flat vectors in blob order (|b| = 0: the absolute error)."""
    out = {}
    for k, s in slices().items():
        nb = float(np.linalg.norm(np.asarray(b[s], dtype=np.float64)))
        out[k] = float(np.linalg.norm(np.asarray(a[s], dtype=np.float64) - np.asarray(b[s], dtype=np.float64))) / (nb if nb > 0 else 1.0)
    return out
