"""Float64 restatement of the learner (PokerQNetwork, environments/Poker/Player.py:178-298 as qnetwork.py implements it)
with an entrywise a-priori bound on |fp32 kernel - float64| next to every value.  A test helper, used by
tests/test_qnet_ref64.py (the bounds themselves, on the CPU) and the GPU suites that hold csrc/qnet.hip to it.

What is restated
  forward   state_dim -> 128 -> 128 -> 64 -> 32 -> n_actions, GELU with the exact erf after the four hidden layers;
            train mode multiplies the outputs of hidden layers 2 and 3 by keep * s, s = 1 / (1 - p), keep the Philox
            draws of the kernels (oracle/qnet_oracle.c: oracle_qnet_keep_masks, bit for bit).
  act       epsilon-greedy: explore = unit(x) < epsilon, uniform action floor(y * n / 2^32), x, y words 0 and 1 of
            Philox4x32-10(seed, table_id0 + row, step); otherwise the first maximal Q.
  training  target = r + gamma * max_a' Q_target(s') * (1 - done); loss = mean (Q(s, a) - target)^2 over the valid rows
            (row_mask and status column 12 in {0, 2}); gradient SUM G of sum_r (Q - target)^2 (what the kernel keeps in
            its gradient buffer); AdamW (torch semantics) on G * min(1, 1 / (|G| / n + 1e-6)) / n, bias correction at
            step t, decoupled weight decay; the target takes the parameters every update_freq optimizer steps.
  Hyperparameters (gamma, p, lr, wd, betas, eps) enter as the fp32 numbers the kernel is handed: the reference states the
  operation the kernel is asked to compute, and the rounding of a constant is not charged to the kernel.

The bounds (u = 2^-24, gamma_k = k u / (1 - k u); all quantities are arrays, |.| and inequalities entrywise)
  Sums.  A k-term fp32 dot product or sum, any order, any association (tiles, MFMA chains, atomics, a reduction tree),
    with each product rounded once, is off from the exact value by at most gamma_k * sum |terms| (Higham, Accuracy and
    Stability, 3.1 and 4.2).  Inputs that already carry an error e are charged |W| e on top: everything below is the
    rounding of this operation plus the propagation of what came in.
  Layer.  z = W h + b computed from h~ = h + dh: the rounding of this layer alone is
      rho = gamma_{n+1} (|W| m_h + |b|),  m_h = |h| + e_h (a bound on |h~|).
  GELU.  The kernel's cdf 0.5 (1 + erf(z / sqrt 2)) is either the library erff (<= 2 ulp) or Abramowitz-Stegun 7.1.26
    (|erf error| <= 1.5e-7) evaluated with fp32 fmas (qnet_device.h: gelu_pair).  Rounding of that evaluation: the
    polynomial sum_i a_i t^i has sum |a_i| <= 4.47 at t <= 1, five fma roundings plus the error of t (rcp, 1 ulp, and
    the rounding of its argument: 2 u) give at most 4.47 * 8 u = 36 u relative to exp(-z^2/2) <= 1; the exponential
    (argument rounded twice, exp2 1 ulp) adds (2 + 0.72 z^2) u exp(-z^2 / 2) <= 3 u; 1 - poly e and the final fma to
    the cdf round twice more: the cdf is off by at most 0.5 * (1.5e-7 + 40 u) + u = 0.5 * 1.5e-7 + C_CDF u, C_CDF = 21,
    absolutely; y = z * cdf rounds once more.  Taylor with max |gelu''| = 2 phi(0) = 0.7979 -> 0.80:
      gelu~(z + dz) = gelu(z) + gelu'(z) dz + r + ev,  |r| <= 0.4 dz^2,  |ev| <= (0.5 * 1.5e-7 + 21 u) |z| + u |gelu(z)|.
    Dropout: h = gelu * m, m = keep * s.  The kernel's s = fl(1 / fl(1 - p)) is within 2 u of s relatively and the
    product rounds once: 3 u m (|gelu| + |gelu'| e_z + |r| + |ev|) more.  eta = m (|r| + |ev|) (+ that) is the part of
    dh that is not gelu'(z) m dz.
  Propagation.  With the exact D_l = m_l gelu'(z_l) the errors obey the LINEAR recursion
      dz_{l+1} = W_{l+1} (D_l dz_l + eta_l) + rho_{l+1}
    (exact: r and ev sit in eta), so dz_L = sum_l J_{L<-z_l} rho_l + sum_l J_{L<-h_l} eta_l with the exact Jacobians
    J_{L<-h_l} = W_L D_{L-1} W_{L-1} ... W_{l+1},  J_{L<-z_l} = J_{L<-h_l} D_l, and
      e_z_L = rho_L + sum_{l<L} |J_{L<-z_l}| rho_l + |J_{L<-h_l}| eta_l,   e_h_l = m |gelu'| e_z_l + eta_l,
    where eta_l uses e_z_l for |r| <= 0.4 e_z_l^2.  (Propagating |W| e_h layer by layer instead is as rigorous but
    assumes every error aligned with every weight's sign: at real observation magnitudes it grows 6x per layer and
    left Q's bound at half of |Q|.)
  TD error.  e_q from the layer recursion (no GELU on the output layer); max is 1-Lipschitz in the sup norm, so
    e_max = max_a e_q'(a).  target = r + gamma max (1 - d) and td = q_a - target take three roundings:
      e_td = e_q(a) + gamma (1 - d) e_max + 3 u (|q_a| + |r| + gamma |max|).
  Backward.  d_5 = 2 td at the taken action (times 2 is exact).  g_l = W_{l+1}^T d_{l+1} (k = fan-out terms):
      e_g = gamma_k |W^T| (|d| + e_d) + |W^T| e_d,
    gelu'(z) = cdf + z phi(z): Taylor with max |gelu'''| = max phi |z^3 - 4 z| = 0.78 -> 0.80, and the cdf as above,
    the density term z phi(z) e with exp2 and the fma 4 u more:
      e_gelu' = min(|gelu''(z)| + 0.4 e_z, 0.80) e_z + 0.5 * 1.5e-7 + 25 u, and with the dropout factor as for h.
    (The backward pass keeps the entrywise |W^T| recursion: its bound is looser than the forward's.)  d_l = g_l * gd_l:  e_d = |g| e_gd + |gd| e_g + e_g e_gd + u (|g| + e_g)(|gd| + e_gd).
  Gradient.  G_l = sum_r d_l,r h_{l-1,r}^T: R products summed in any order:
      e_G = gamma_R sum_r (|d| + e_d)(|h| + e_h) + sum_r (|d| e_h + e_d |h| + e_d e_h)   (biases: h = 1, e_h = 0).
  Reports.  loss = sq / n, sq = sum td^2:  e_sq = sum (2 |td| e_td + e_td^2) + gamma_R sum (|td| + e_td)^2, and 2 u
    for the division.  norm = sqrt(sum G^2) / n: |(|G~| - |G|)| <= |e_G|_2 (triangle inequality), the device's sum of
    squares is within gamma_N (N parameters) relatively, the square root and the two divisions 3 u more.
  AdamW (from the device's own gradient sum, moments and parameters, so that nothing of the gradient's error hides a
    slip of the optimizer): with rho = gamma_N / 2 + 5 u the relative error of the clipping factor
      e_g  = |g| (rho + u)
      e_m  = (1 - b1) e_g + 3 u (b1 |m| + (1 - b1) |g|)             (1 - b1 is exact: Sterbenz)
      e_v  = (1 - b2)(2 |g| e_g + e_g^2) + 4 u (b2 v + (1 - b2) g^2)
      bias corrections 1 - b^t: powf 2 u of b^t plus one rounding; the square root of the second halves its error;
      den  = sqrt(v) / sqrt(bc2) + eps, e_den from e_sqrt(v) = min(e_v / sqrt v, sqrt e_v), the relative error of
             sqrt(bc2) and three roundings;
      U    = lr / bc1 * m / den:  e_U = step (e_m / den_lo + |m| e_den / (den den_lo)) + |U| (e_bc1 / bc1 + 3 u),
             den_lo = max(den - e_den, eps (1 - u)) (the kernel's den is a rounded sum of sqrt(v~) / . >= 0 and
             eps, so it is at least eps (1 - u));
      p'   = p (1 - lr wd) - U:  e_p = 4 u |p| + e_U + u |p'|.
    Underflow: the kernels flush denormals, so each rounding may also lose up to 2^-126 absolutely (one such term per
    rounding in rho, the gradient sums, e_g, e_m, e_v and e_p); a gradient entry of 1e-45 leaves exp_avg at 0 where float64 has 1e-48.
  No factor in this file is a safety margin: each constant is the count of roundings or the analytic maximum named
  next to it.
"""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24
UF = 2.0 ** -126         # with denormals flushed, a rounding may also lose up to the smallest normal number absolutely
AS_ERF = 1.5e-7          # Abramowitz-Stegun 7.1.26
GELU2_LIP = 0.80         # max |gelu''(z)| = 2 phi(0) = 0.7979
GELU3_LIP = 0.80         # max |gelu'''(z)| = max phi(z) |z^3 - 4 z| = 0.78 (z = 0.74)
C_CDF = 21               # absolute error of the kernel's cdf in u (module docstring)
C_DCDF = 25              # ... of its gelu'
HIDDEN = (128, 128, 64, 32)


def gam(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def f32(x) -> float:
    return float(np.float32(x))


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(torch.as_tensor(z) / np.sqrt(2.0)).numpy())


def dgelu64(z):
    zt = torch.as_tensor(z)
    return (0.5 * (1.0 + torch.erf(zt / np.sqrt(2.0))) + zt * torch.exp(-0.5 * zt * zt) / np.sqrt(2.0 * np.pi)).numpy()


def d2gelu64(z):
    return np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) * (2.0 - z * z)


def split(flat, state_dim, n_actions):
    """flat (w1, b1, ..., w5, b5) -> ([W1..W5], [b1..b5]) in float64."""
    flat = np.asarray(flat, dtype=np.float64)
    dims = [state_dim, *HIDDEN, n_actions]
    ws, bs, o = [], [], 0
    for l in range(5):
        n = dims[l + 1] * dims[l]
        ws.append(flat[o:o + n].reshape(dims[l + 1], dims[l])); o += n
        bs.append(flat[o:o + dims[l + 1]]); o += dims[l + 1]
    assert o == flat.size, "flat parameter count does not match the shapes"
    return ws, bs


def join(ws, bs):
    return np.concatenate([np.concatenate([w.ravel(), b.ravel()]) for w, b in zip(ws, bs)])


def param_count(state_dim, n_actions):
    dims = [state_dim, *HIDDEN, n_actions]
    return sum(dims[l + 1] * dims[l] + dims[l + 1] for l in range(5))


def keep_masks(seed, step, table_ids, p=0.1):
    """The kernels' dropout keeps -> (keep2 bool[n,128], keep3 bool[n,64])."""
    from oracle import oracle as orc
    k = orc.qnet_keep_masks(seed, step, table_ids, p)
    return k[:, :128], k[:, 128:]


def forward(ws, bs, x, keeps=None, p=0.1, chunk=512):
    """Float64 forward with bounds.  keeps None: eval mode.  Returns dict(q, e_q, z, e_z, h, e_h, gelu) with lists per layer:
    h[0] = x, z[l] / h[l + 1] for layer l = 0..4 (h[5] = q).  The errors are propagated through the exact Jacobians
    (module docstring: Propagation), row chunk by row chunk."""
    x = np.asarray(x, dtype=np.float64)
    s = 1.0 / (1.0 - f32(p))
    n = x.shape[0]
    h, zs, gl, ms = [x], [], [], []
    for l in range(5):
        z = h[-1] @ ws[l].T + bs[l]
        zs.append(z)
        if l == 4:
            h.append(z)
            break
        g = gelu64(z)
        m = keeps[l - 1].astype(np.float64) * s if (keeps is not None and l in (1, 2)) else np.ones((1, z.shape[1]))
        gl.append(g); ms.append(m)
        h.append(g * m)
    e_z = [np.zeros_like(z) for z in zs]
    e_h = [np.zeros_like(x)] + [np.zeros_like(z) for z in zs]
    Wt = [torch.from_numpy(w) for w in ws]
    aW = [np.abs(w) for w in ws]
    for c0 in range(0, n, chunk):
        sl = slice(c0, min(n, c0 + chunk))
        rho, eta, D = [], [], []
        for L in range(5):
            hp, ep = h[L][sl], e_h[L][sl]
            r = gam(ws[L].shape[1] + 1) * ((np.abs(hp) + ep) @ aW[L].T + np.abs(bs[L])) + (ws[L].shape[1] + 1) * UF
            rho.append(torch.from_numpy(r))
            ez = r.copy()
            M = Wt[L].expand(r.shape[0], *Wt[L].shape)                     # d z_L / d h_{L-1}
            for l in range(L - 1, -1, -1):
                ez += torch.bmm(M.abs(), eta[l][:, :, None])[:, :, 0].numpy()
                M = M * D[l][:, None, :]                                   # d z_L / d z_l
                ez += torch.bmm(M.abs(), rho[l][:, :, None])[:, :, 0].numpy()
                if l > 0:
                    M = torch.matmul(M, Wt[l])                             # d z_L / d h_{l-1}
            e_z[L][sl] = ez
            if L == 4:
                e_h[5][sl] = ez
                break
            z, g = zs[L][sl], gl[L][sl]
            m = np.broadcast_to(ms[L][sl] if ms[L].shape[0] > 1 else ms[L], z.shape)
            dg = dgelu64(z)
            rem = 0.5 * GELU2_LIP * ez * ez
            ev = (0.5 * AS_ERF + C_CDF * U) * np.abs(z) + U * np.abs(g)
            et = m * (rem + ev)
            if keeps is not None and L in (1, 2):
                et = et + 3 * U * m * (np.abs(g) + np.abs(dg) * ez + rem + ev)
            eta.append(torch.from_numpy(np.ascontiguousarray(et)))
            D.append(torch.from_numpy(np.ascontiguousarray(m * dg)))
            e_h[L + 1][sl] = m * np.abs(dg) * ez + et
    return dict(q=h[5], e_q=e_h[5], z=zs, e_z=e_z, h=h, e_h=e_h, gelu=gl)


def valid_rows(states, row_mask=None):
    st = np.asarray(states)[:, 12]
    v = (st == 0) | (st == 2)
    if row_mask is not None:
        v &= np.asarray(row_mask, dtype=bool)
    return v


def train_grads(params, target, state_dim, n_actions, states, actions, rewards, next_states, dones, row_mask=None,
                gamma=0.95, p=0.1, seed=0, step=0, table_id0=0):
    """One training step's gradient SUM, loss and norm with bounds.  p = 0: eval-mode forward (network.eval()).
    Rows are those of the batch (dropout keyed by table_id0 + row index, as the kernel does)."""
    ws, bs = split(params, state_dim, n_actions)
    tws, tbs = split(target, state_dim, n_actions)
    v = valid_rows(states, row_mask)
    idx = np.flatnonzero(v)
    R = idx.size
    out = dict(count=R, grad=np.zeros(param_count(state_dim, n_actions)), e_grad=np.zeros(param_count(state_dim, n_actions)),
               sq=0.0, e_sq=0.0, loss=0.0, e_loss=0.0, norm=0.0, e_norm=0.0, rows=idx)
    if R == 0:
        return out
    x = np.asarray(states, dtype=np.float64)[idx]
    xn = np.asarray(next_states, dtype=np.float64)[idx]
    a = np.asarray(actions, dtype=np.int64)[idx]
    r = np.asarray(rewards, dtype=np.float64)[idx]
    nd = 1.0 - np.asarray(dones, dtype=np.float64)[idx]
    gm = f32(gamma)
    keeps = keep_masks(seed, step, np.uint64(table_id0) + idx.astype(np.uint64), p) if p > 0 else None
    fw = forward(ws, bs, x, keeps, p)
    ft = forward(tws, tbs, xn)
    qa = fw["q"][np.arange(R), a]
    e_qa = fw["e_q"][np.arange(R), a]
    mx = ft["q"].max(axis=1)
    e_mx = ft["e_q"].max(axis=1)
    tgt = r + gm * mx * nd
    td = qa - tgt
    e_td = e_qa + gm * nd * e_mx + 3 * U * (np.abs(qa) + np.abs(r) + gm * np.abs(mx))
    out.update(td=td, e_td=e_td, q=fw["q"], e_q=fw["e_q"], target=tgt, fw=fw)
    # backward
    s = 1.0 / (1.0 - f32(p))
    d = np.zeros((R, n_actions)); d[np.arange(R), a] = 2 * td
    e_d = np.zeros((R, n_actions)); e_d[np.arange(R), a] = 2 * e_td
    gW, eW, gB, eB = [None] * 5, [None] * 5, [None] * 5, [None] * 5
    for l in range(4, -1, -1):
        h, e_h = fw["h"][l], fw["e_h"][l]
        ad, ah = np.abs(d), np.abs(h)
        gW[l] = d.T @ h
        eW[l] = gam(R) * ((ad + e_d).T @ (ah + e_h)) + ad.T @ e_h + e_d.T @ ah + e_d.T @ e_h + 2 * R * UF
        gB[l] = d.sum(axis=0)
        eB[l] = gam(R) * (ad + e_d).sum(axis=0) + e_d.sum(axis=0) + R * UF
        if l == 0:
            break
        W = ws[l]; aW = np.abs(W)
        g = d @ W
        e_g = gam(W.shape[0]) * ((ad + e_d) @ aW) + e_d @ aW
        z, e_z = fw["z"][l - 1], fw["e_z"][l - 1]
        gd = dgelu64(z)
        e_gd = np.minimum(np.abs(d2gelu64(z)) + 0.5 * GELU3_LIP * e_z, GELU2_LIP) * e_z + 0.5 * AS_ERF + C_DCDF * U
        if p > 0 and l - 1 in (1, 2):
            m = keeps[l - 2].astype(np.float64) * s
            e_gd = m * (e_gd + 3 * U * (np.abs(gd) + e_gd))
            gd = gd * m
        d = g * gd
        e_d = np.abs(g) * e_gd + np.abs(gd) * e_g + e_g * e_gd + U * (np.abs(g) + e_g) * (np.abs(gd) + e_gd)
    out["grad"] = join(gW, gB)
    out["e_grad"] = join(eW, eB)
    sq = float((td ** 2).sum())
    e_sq = float((2 * np.abs(td) * e_td + e_td ** 2).sum() + gam(R) * ((np.abs(td) + e_td) ** 2).sum())
    out.update(sq=sq, e_sq=e_sq, loss=sq / R, e_loss=e_sq / R + 2 * U * (sq + e_sq) / R)
    G, eG = out["grad"], out["e_grad"]
    nG = float(np.sqrt((G ** 2).sum()))
    neG = float(np.sqrt((eG ** 2).sum()))
    out.update(norm=nG / R, e_norm=neG / R + (gam(G.size) / 2 + 3 * U) * (nG + neG) / R)
    return out


def adamw(params, target, grad_sum, m, v, count, t, lr, wd, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, update_freq=0):
    """AdamW from the DEVICE's gradient sum (fp32 array), moments and parameters, in float64, with bounds.
    Returns dict(params, target, m, v, e_params, e_m, e_v, coef, norm, synced)."""
    p = np.asarray(params, dtype=np.float64); G = np.asarray(grad_sum, dtype=np.float64)
    m0 = np.asarray(m, dtype=np.float64); v0 = np.asarray(v, dtype=np.float64)
    lr, wd, b1, b2, eps = f32(lr), f32(wd), f32(beta1), f32(beta2), f32(eps)
    if count <= 0:
        z = np.zeros_like(p)
        return dict(params=p, target=np.asarray(target, dtype=np.float64), m=m0, v=v0, e_params=z, e_m=z, e_v=z, coef=0.0, norm=0.0,
                    synced=False)
    n = float(count)
    norm = float(np.sqrt((G ** 2).sum())) / n
    coef = min(max_norm / (norm + f32(1e-6)), 1.0) / n
    rho = gam(G.size) / 2 + 5 * U
    g = G * coef
    e_g = np.abs(g) * (rho + U) + UF
    mn = b1 * m0 + (1 - b1) * g
    vn = b2 * v0 + (1 - b2) * g * g
    e_m = (1 - b1) * e_g + 3 * U * (b1 * np.abs(m0) + (1 - b1) * np.abs(g)) + 3 * UF
    e_v = (1 - b2) * (2 * np.abs(g) * e_g + e_g ** 2) + 4 * U * (b2 * v0 + (1 - b2) * g * g) + 4 * UF
    bt1, bt2 = b1 ** t, b2 ** t
    bc1, bc2 = 1 - bt1, 1 - bt2
    e_bc1, e_bc2 = 2 * U * bt1 + U * bc1, 2 * U * bt2 + U * bc2
    rel_bc2s = 0.5 * e_bc2 / bc2 + U
    bc2s = np.sqrt(bc2)
    sv = np.sqrt(vn)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_sv = np.where(sv > 0, np.minimum(e_v / np.where(sv > 0, sv, 1.0), np.sqrt(e_v)), np.sqrt(e_v))
    den = sv / bc2s + eps
    e_den = e_sv / bc2s + (sv / bc2s) * rel_bc2s + 3 * U * den
    den_lo = np.maximum(den - e_den, eps * (1 - U))          # the kernel's den is at least fl(0 + eps) = eps
    step = lr / bc1
    upd = step * mn / den
    e_upd = step * (e_m / den_lo + np.abs(mn) * e_den / (den * den_lo)) + np.abs(upd) * (e_bc1 / bc1 + 3 * U)
    pn = p * (1 - lr * wd) - upd
    e_p = 4 * U * np.abs(p) + e_upd + U * np.abs(pn) + 4 * UF
    synced = update_freq > 0 and t % update_freq == 0
    tn = pn.copy() if synced else np.asarray(target, dtype=np.float64)
    return dict(params=pn, target=tn, m=mn, v=vn, e_params=e_p, e_m=e_m, e_v=e_v, coef=coef, norm=norm, synced=synced)


def explore_draws(n_rows, n_actions, epsilon, seed, step, table_id0):
    """(explore bool[n], uniform action int64[n]) of the act kernels' Philox draws for rows 0..n-1, through the oracle's
    own epsilon-greedy (two calls: greedy 0 and greedy 1 everywhere; a row explored iff both calls pick the same action)."""
    from oracle import oracle as orc
    if n_actions == 1:
        return np.zeros(n_rows, dtype=bool), np.zeros(n_rows, dtype=np.int64)
    qa = np.full((n_rows, n_actions), -1.0, dtype=np.float32); qa[:, 0] = 0.0
    qb = np.full((n_rows, n_actions), -1.0, dtype=np.float32); qb[:, 1] = 0.0
    A = np.zeros(n_rows, dtype=np.int64); B = np.zeros(n_rows, dtype=np.int64)
    orc.qnet_act(qa, None, 0, epsilon, seed, step, table_id0, A)
    orc.qnet_act(qb, None, 0, epsilon, seed, step, table_id0, B)
    return A == B, A


def greedy_candidates(q, e_q):
    """bool[n, A]: the actions an fp32 evaluation within the bounds may pick (Q_a + e_a >= max_b (Q_b - e_b)), and the
    float64 argmax."""
    lo = (q - e_q).max(axis=1, keepdims=True)
    return (q + e_q) >= lo, q.argmax(axis=1)


def check_actions(got, q, e_q, explore, uniform, rows=None, ctx=""):
    """The action rules: explored rows exact; others exact where the float64 top-two gap exceeds the sum of their bounds,
    else one of the candidates within the band.  Returns the number of rows decided exactly."""
    got = np.asarray(got)
    rows = np.arange(q.shape[0]) if rows is None else np.asarray(rows)
    cand, arg = greedy_candidates(q[rows], e_q[rows])
    g, ex, un = got[rows], explore[rows], uniform[rows]
    bad_ex = ex & (g != un)
    assert not bad_ex.any(), f"{ctx}: explored rows differ, first at row {rows[np.flatnonzero(bad_ex)[0]]}"
    single = cand.sum(axis=1) == 1
    bad = ~ex & single & (g != arg)
    assert not bad.any(), (f"{ctx}: {int(bad.sum())} clear greedy rows differ, first at row {rows[np.flatnonzero(bad)[0]]}: "
                           f"got {g[bad][0]} want {arg[bad][0]}")
    ok = (g >= 0) & (g < q.shape[1])
    inband = np.zeros_like(ok)
    inband[ok] = cand[np.flatnonzero(ok), g[ok]]
    bad = ~ex & ~inband
    assert not bad.any(), f"{ctx}: {int(bad.sum())} rows pick an action outside the band, first at row {rows[np.flatnonzero(bad)[0]]}"
    return int((~ex & single).sum())


def assert_within(got, want, bound, what):
    """|got - want| <= bound entrywise; returns the ratios |got - want| / bound (0 where both are 0)."""
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64); bound = np.asarray(bound, dtype=np.float64)
    err = np.abs(got - want)
    bad = err > bound
    if bad.any():
        i = int(np.flatnonzero(bad.ravel())[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries outside the bound; first at flat index {i}: "
                             f"got {got.ravel()[i]!r} want {want.ravel()[i]!r} err {err.ravel()[i]:.3g} bound {bound.ravel()[i]:.3g}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)


def within(got, want, bound):
    return bool((np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) <= bound).all())


def ratio_stats(r):
    r = np.asarray(r).ravel()
    r = r[r > 0]
    return (float(np.median(r)), float(r.max())) if r.size else (0.0, 0.0)


def oracle_transitions(n_games, max_players, n_players=None, episodes=2, steps=6, seed=0):
    """Real observation rows: (states, next_states, rewards, dones) of OraclePokerEnv roll-outs (bit-identical to PokerGPU's,
    tests/test_poker_gpu_parity.py) with random actions, stacks carried over `episodes` resets; the rows of the last
    `steps` steps of the last episode are stacked."""
    from oracle import oracle as orc
    P = n_players or max_players
    env = orc.OraclePokerEnv(n_players=P, max_players=max_players, n_games=n_games, starting_bbs=100, max_bbs=1000, w1=.5, w2=.3,
                             K=100, alpha=50)
    rng = np.random.default_rng(seed)
    S, NS, R, D = [], [], [], []
    for ep in range(episodes):
        decks = (rng.random((n_games, 52)).argsort(axis=1) + 1).astype(np.int32)
        obs, _ = env.reset(options={"prefixed_decks": decks, "rotation": ep})
        for _ in range(steps):
            before = obs.copy()
            obs, rew, done, _, _ = env.step(rng.integers(0, 13, n_games))
            if ep == episodes - 1:
                S.append(before); NS.append(obs.copy()); R.append(rew.copy()); D.append(done.copy())
    return np.concatenate(S), np.concatenate(NS), np.concatenate(R), np.concatenate(D)
