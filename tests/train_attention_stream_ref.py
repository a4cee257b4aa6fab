"""float64 closed-form forward and backward of the Attention core (attention.py:62-72), head by head and without an autograd tape: the
reference of the streaming training kernels at token counts where a tape over all heads would not fit (four N x N float64 matrices at a
time, 0.6 GB at N = 4225).  tests/test_train_attention_stream_ref.py pins it to tests/train_op_refs.attention + torch.autograd.

    S = q k^T / sqrt(32)     P = softmax_j(S)     Pd = P keep / (1 - p)     out = Pd v
    dPd = dout v^T           dP = dPd keep / (1 - p)                        D_i = sum_j P_ij dP_ij
    dS = P (dP - D)          dq = dS k / sqrt(32)    dk = dS^T q / sqrt(32)    dv = Pd^T dout
"""
import torch

HEADS, DH, HID = 4, 32, 128


def attention_fwd_bwd64(qkv, dout, keep=None, p=0.0):
    """qkv (nb, N, 384), dout (nb, N, 128), keep (nb, 4, N, N) or None -> {"y" (nb, N, 128), "dq", "dk", "dv" (nb, N, 128)}, float64."""
    nb, n, _ = qkv.shape
    x, g = qkv.double(), dout.double().reshape(nb, n, HEADS, DH)
    q, k, v = (x[:, :, i * HID:(i + 1) * HID].reshape(nb, n, HEADS, DH) for i in range(3))
    out = {name: torch.empty(nb, n, HEADS, DH, dtype=torch.float64) for name in ("y", "dq", "dk", "dv")}
    scale, sc = DH ** -0.5, 1.0 / (1.0 - p)
    for b in range(nb):
        for h in range(HEADS):
            qh, kh, vh, gh = q[b, :, h], k[b, :, h], v[b, :, h], g[b, :, h]
            P = torch.softmax(qh @ kh.T * scale, dim=-1)
            dP = gh @ vh.T
            if keep is not None:
                kp = keep[b, h].double() * sc
                dP *= kp
                Pd = P * kp
                del kp
            else:
                Pd = P
            out["y"][b, :, h] = Pd @ vh
            out["dv"][b, :, h] = Pd.T @ gh
            del Pd
            dP -= (P * dP).sum(-1, keepdim=True)
            dP *= P  # dS
            out["dq"][b, :, h] = dP @ kh * scale
            out["dk"][b, :, h] = dP.T @ qh * scale
    return {name: t.reshape(nb, n, HID) for name, t in out.items()}
