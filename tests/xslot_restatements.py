"""The fused xSlot head (csrc/xslot_fwd.hip, xslot_bwd.hip, xslot_small_*.h) restated on the host, returning EVERY row the kernels
store -- not only the parameter gradients the rows are contracted into.  The maths is oracle/xslot_manual.py (forward and
hand-derived backward, proved against autograd there and in tests/test_xslot_instances_cpu.py); here it runs in torch at a chosen
dtype: float64 is the truth, float32 the yardstick of what plain fp32 arithmetic loses on the same inputs.

Index conventions are those of the CONSUMERS of the rows, sloter/utils/slot_attention.py (_param_grads):
  * states[k], k = 0..T-2: the slots entering iteration k + 1 (iteration 0 starts from the initial slots, which are not saved);
  * U[t], dgi[t], dgh[t], t = 0..T-2: the GRU call that closes iteration t -- its input, and the gradients of its input-side and
    hidden-side gate pre-activations in nn.GRU's block order r | z | n:  dW_ih = sum_t dgi[t]^T U[t],  dW_hh = sum_t dgh[t]^T h_t
    with h_0 = the initial slots (the same rows for every image) and h_t = states[t - 1];
  * H[l] = the INPUT of to_k layer l (H[0] = X + PE), dZ[l] = the gradient of its pre-activation:  dW_l = dZ[l]^T H[l];
  * ds0[b] = the gradient of the initial slots through image b (their sum over the batch is the parameter's gradient).
Test infrastructure only: nothing here is imported by the package."""
import torch


def head(P, X, PE, spc, T, loss_status, dlogits, g_area, dtype=torch.float64):
    """P: tok_w [L x (d, d)], tok_b [L x (d)], slots0 (S, d), w_ih, w_hh (3d, d), b_ih, b_hh (3d).  X: (B, N, d) post-ReLU tokens,
    PE: (N, d), dlogits: (B, S / spc), g_area: dL/d(sum of the last iteration's attention), a float (0.0 = a null g_area_sum).
    Returns a dict of tensors / lists of tensors at `dtype` (see the module docstring), plus the quantities the input conditions of
    tests/xslot_cases.py are stated on: Z (to_k pre-activations), r (per iteration, the row sums the attention divides by)."""
    c = lambda t: t.to(dtype)
    X, PE, dlogits = c(X), c(PE), c(dlogits)
    tw, tb = [c(w) for w in P["tok_w"]], [c(b) for b in P["tok_b"]]
    s0, w_ih, w_hh, b_ih, b_hh = c(P["slots0"]), c(P["w_ih"]), c(P["w_hh"]), c(P["b_ih"]), c(P["b_hh"])
    B, N, d = X.shape
    S, L = s0.shape[0], len(tw)
    scale = d ** -0.5
    # ---- forward
    H, Z = [X + PE], []
    for l in range(L):
        Z.append(H[l] @ tw[l].t() + tb[l])
        if l < L - 1:
            H.append(torch.relu(Z[l]))
    K = Z[-1]
    s = s0.expand(B, S, d)
    ent, it = [], []                                   # slots entering iteration t; what iteration t computed
    for t in range(T):
        ent.append(s)
        D = torch.einsum("bid,bjd->bij", s, K) * scale
        r = D.sum(2, keepdim=True)
        tau = r.sum(1, keepdim=True)
        A = torch.sigmoid(D / r * tau)
        U = torch.einsum("bij,bjd->bid", A, X) / d
        rec = dict(D=D, r=r, tau=tau, A=A, U=U)
        if t < T - 1:
            gi, gh = U @ w_ih.t() + b_ih, s @ w_hh.t() + b_hh
            rg = torch.sigmoid(gi[..., :d] + gh[..., :d])
            zg = torch.sigmoid(gi[..., d:2 * d] + gh[..., d:2 * d])
            hn = gh[..., 2 * d:]
            ng = torch.tanh(gi[..., 2 * d:] + rg * hn)
            rec.update(rg=rg, zg=zg, ng=ng, hn=hn)
            s = (1 - zg) * ng + zg * s
        it.append(rec)
    A, U = it[-1]["A"], it[-1]["U"]
    logits = loss_status * U.reshape(B, S // spc, spc, d).sum((2, 3))
    out = dict(K=K, H=H, Z=Z, states=ent[1:], attn=A, area_part=A.sum((1, 2)), logits=logits, r=[q["r"] for q in it])
    # ---- backward: dL/dU_T[s, k] = loss_status * dlogits[class of s]
    dU = (loss_status * dlogits).repeat_interleave(spc, dim=1)[:, :, None].expand(B, S, d)
    ds = torch.zeros(B, S, d, dtype=dtype)
    dK, dX = torch.zeros_like(K), torch.zeros_like(X)
    Us, dgis, dghs = [None] * (T - 1), [None] * (T - 1), [None] * (T - 1)
    for t in range(T - 1, -1, -1):
        q, sp = it[t], ent[t]
        dh_prev = torch.zeros_like(sp)
        if t < T - 1:
            rg, zg, ng, hn = q["rg"], q["zg"], q["ng"], q["hn"]
            da_n = ds * (1 - zg) * (1 - ng * ng)
            da_r = da_n * hn * rg * (1 - rg)
            da_z = ds * (sp - ng) * zg * (1 - zg)
            dgi = torch.cat([da_r, da_z, da_n], -1)
            dgh = torch.cat([da_r, da_z, da_n * rg], -1)
            dU = dgi @ w_ih
            dh_prev = ds * zg + dgh @ w_hh
            Us[t], dgis[t], dghs[t] = q["U"], dgi, dgh
        dA = torch.einsum("bid,bjd->bij", dU, X) / d
        if t == T - 1:
            dA = dA + g_area
        dX = dX + torch.einsum("bij,bid->bjd", q["A"], dU) / d
        G = dA * q["A"] * (1 - q["A"])
        g = (G * q["D"]).sum(2, keepdim=True)
        c0 = (g / q["r"]).sum(1, keepdim=True)
        dD = G * q["tau"] / q["r"] - g * q["tau"] / (q["r"] * q["r"]) + c0
        ds = scale * torch.einsum("bij,bjd->bid", dD, K) + dh_prev
        dK = dK + scale * torch.einsum("bij,bid->bjd", dD, sp)
    dZ, dz = [None] * L, dK
    for l in range(L - 1, -1, -1):
        if l < L - 1:
            dz = dz * (H[l + 1] > 0)
        dZ[l] = dz
        dz = dz @ tw[l]
    out.update(U=Us, dgi=dgis, dgh=dghs, ds0=ds, dZ=dZ, dX=dX + dz)
    return out


def param_grads(rows, slots0, H, states):
    """The parameter gradients as sloter/utils/slot_attention.py forms them from the rows a backward emitted (rows: U, dgi, dgh,
    ds0, dZ) and the forward's saved H / states -- in fp64 whatever the rows' dtype, so that what is compared is the rows."""
    f = lambda t: t.double()
    d = slots0.shape[1]
    g = {"slots0": f(rows["ds0"]).sum(0)}
    for name, shape in (("w_ih", (3 * d, d)), ("w_hh", (3 * d, d)), ("b_ih", (3 * d,)), ("b_hh", (3 * d,))):
        g[name] = torch.zeros(shape, dtype=torch.float64)
    for t in range(len(rows["dgi"])):
        dgi, dgh = f(rows["dgi"][t]), f(rows["dgh"][t])
        h = f(slots0).expand(dgh.shape[0], -1, -1) if t == 0 else f(states[t - 1])
        g["w_ih"] += torch.einsum("bsg,bsd->gd", dgi, f(rows["U"][t]))
        g["w_hh"] += torch.einsum("bsg,bsd->gd", dgh, h)
        g["b_ih"] += dgi.sum((0, 1))
        g["b_hh"] += dgh.sum((0, 1))
    for l, dz in enumerate(rows["dZ"]):
        g["tok_w%d" % l] = torch.einsum("bno,bni->oi", f(dz), f(H[l]))
        g["tok_b%d" % l] = f(dz).sum((0, 1))
    return g
