"""Float64 restatement of MotionVectorVSR's reconstruction (reference models/mvvsr_arch.py:95-105) in the two forms
csrc/mv_recon.h is built on, with its analytic backward.  TEST INFRASTRUCTURE (no GPU, no product code).

For frame i, c = cat(feat_b[i], feat_f[i]):   u = lrelu_0.1(W_fu c + b_fu);   D = conv_transpose2d(u, W_last, b_last, stride 4);
out = interpolate(D, (4h, 4w), bilinear) + interpolate(x_i, (4h, 4w), bilinear).

  phase form   D[o, 4y+i, 4x+j] = b[o] + E[o,i,j](y,x) + [i=0] E[o,4,j](y-1,x) + [j=0] E[o,i,4](y,x-1) + [i=j=0] E[o,4,4](y-1,x-1),
               E[o,ky,kx](y,x) = sum_c u[c,y,x] W[c,o,ky,kx], zero outside the h x w image (so row 4h / column 4w get the k = 4 taps only)
  blend        out[d] = (1 - l_d) D[d] + l_d D[d+1], l_d = (2d+1)/(8h) rows, (2d+1)/(8w) columns
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.mfma_emu import rnd

SLOPE = 0.1


def fuse(c, w_fu, b_fu):
    pre = torch.einsum("oi,nihw->nohw", w_fu.reshape(w_fu.shape[0], -1), c) + b_fu.view(1, -1, 1, 1)
    return torch.where(pre > 0, pre, SLOPE * pre)


def _shift(a, dy, dx):
    """a[..., y - dy, x - dx] with zeros shifted in (dy, dx in {0, 1})"""
    return F.pad(a, (dx, 0, dy, 0))[..., :a.shape[-2], :a.shape[-1]]


def phase_D(u, w_last, b_last):
    n, _, h, w = u.shape
    E = torch.einsum("nchw,cokl->noklhw", u, w_last)
    Ez = F.pad(E, (0, 1, 0, 1))                       # LR row h and column w: u = 0
    D = u.new_zeros(n, 3, 4 * (h + 1), 4 * (w + 1))
    for i in range(4):
        for j in range(4):
            v = Ez[:, :, i, j].clone()
            if i == 0:
                v += _shift(Ez[:, :, 4, j], 1, 0)
            if j == 0:
                v += _shift(Ez[:, :, i, 4], 0, 1)
            if i == 0 and j == 0:
                v += _shift(Ez[:, :, 4, 4], 1, 1)
            D[:, :, i::4, j::4] = v
    return D[:, :, :4 * h + 1, :4 * w + 1] + b_last.view(1, 3, 1, 1)


def lambdas(h, dtype=torch.float64):
    return (2 * torch.arange(4 * h, dtype=dtype) + 1) / (8 * h)


def blend(D):
    h, w = (D.shape[-2] - 1) // 4, (D.shape[-1] - 1) // 4
    ly, lx = lambdas(h, D.dtype).view(-1, 1), lambdas(w, D.dtype).view(1, -1)
    rows = (1 - ly) * D[..., :-1, :] + ly * D[..., 1:, :]
    return (1 - lx) * rows[..., :-1] + lx * rows[..., 1:]


def base(x):
    """x4 bilinear of the frames, align_corners = False"""
    return F.interpolate(x, scale_factor=4, mode="bilinear", align_corners=False)


def forward(fb, ff, x, w_fu, b_fu, w_last, b_last):
    """fb, ff (N, F, h, w), x (N, 3, h, w) -> (out (N, 3, 4h, 4w), c, u, D)"""
    c = torch.cat([fb, ff], 1)
    u = fuse(c, w_fu, b_fu)
    D = phase_D(u, w_last, b_last)
    return blend(D) + base(x), c, u, D


def blend_T(g):
    """dD[d] = (1 - l_d) g[d] + l_{d-1} g[d-1], rows then columns"""
    h, w = g.shape[-2] // 4, g.shape[-1] // 4
    ly, lx = lambdas(h, g.dtype).view(-1, 1), lambdas(w, g.dtype).view(1, -1)
    cols = F.pad((1 - lx) * g, (0, 1)) + F.pad(lx * g, (1, 0))
    return F.pad((1 - ly) * cols, (0, 0, 0, 1)) + F.pad(ly * cols, (0, 0, 1, 0))


def gather_dE(dD):
    """dE[n, o, y, ky, x, kx] = dD[n, o, 4y + ky, 4x + kx]"""
    h, w = (dD.shape[-2] - 1) // 4, (dD.shape[-1] - 1) // 4
    rows = 4 * torch.arange(h).view(-1, 1) + torch.arange(5).view(1, -1)
    cols = 4 * torch.arange(w).view(-1, 1) + torch.arange(5).view(1, -1)
    return dD[:, :, rows[:, :, None, None], cols[None, None, :, :]]


def backward(g, c, u, w_fu, w_last):
    """the transpose of `forward`, no scatter: dict(dc, dW_fu, db_fu, dW_last, db_last, dD, du)"""
    dD = blend_T(g)
    dE = gather_dE(dD)
    du = torch.einsum("nohkwl,cokl->nchw", dE, w_last)
    dpre = du * torch.where(u > 0, torch.ones_like(u), torch.full_like(u, SLOPE))
    wf = w_fu.reshape(w_fu.shape[0], -1)
    return dict(dc=torch.einsum("oi,nohw->nihw", wf, dpre), dW_fu=torch.einsum("nohw,nihw->oi", dpre, c).view_as(w_fu),
                db_fu=dpre.sum((0, 2, 3)), dW_last=torch.einsum("nchw,nohkwl->cokl", u, dE), db_last=dD.sum((0, 2, 3)), dD=dD, du=du)


# ---- lane-level emulation of the 16 x 16 x 32 MFMA as csrc/mv_recon.h uses it (vr_mma32 of csrc/vsr_recon.h) ----
LANE = np.arange(64)


def frag_matrix(blob, first, nm, nk):
    """the A matrix (16 nm, 32 nk) that fragments first .. first + nm nk - 1 of the blob hold: fragment (m, s), lane l, element j
    = A[16 m + (l & 15)][32 s + 8 (l >> 4) + j]"""
    A = np.zeros((16 * nm, 32 * nk))
    fr = np.asarray(blob[first:first + nm * nk * 512], dtype=np.float64).reshape(nm, nk, 64, 8)
    for m in range(nm):
        for s in range(nk):
            for j in range(8):
                A[16 * m + (LANE & 15), 32 * s + 8 * (LANE >> 4) + j] = fr[m, s, :, j]
    return A


def emu_contract(blob, first, nm, nk, B, dtype):
    """sum_k A[row][k] B[k][pixel]: weights and B rounded to the storage type, products summed exactly"""
    return frag_matrix(rnd(blob, dtype), first, nm, nk) @ rnd(B, dtype)
