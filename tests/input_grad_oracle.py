"""CPU oracle of the stem's data gradient (video_dqn_amd/csrc/stem_dgrad.hip): max-pool backward from arg-max codes with the
engine's rounding, and the transposed 7x7 / stride-2 convolution written two ways — the packed-space sum the kernel evaluates and
torch's conv_transpose2d on the 7x7 weights — plus the space-to-depth pack and its inverse.  Plain numpy / torch on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F


def s2d_channel(dy, dx, c):
    """Packed channel of source-pixel offset (dy, dx), colour c (pack_input_kernel, pointwise.hip: (bh * 2 + bw) * 3 + c)."""
    return (dy * 2 + dx) * 3 + c


def pack_s2d(frame):
    """[n, 3, 224, 224] -> [n, 115, 115, 16] as pack_input_kernel lays it out: packed pixel (py, px) holds source pixels
    (2 (py - 2) + bh, 2 (px - 2) + bw); rows / columns 0, 1, 114 and the channels 12..15 are zero."""
    n = frame.shape[0]
    t = torch.zeros((n, 115, 115, 16), dtype=frame.dtype)
    for bh in range(2):
        for bw in range(2):
            for c in range(3):
                t[:, 2:114, 2:114, (bh * 2 + bw) * 3 + c] = frame[:, c, bh::2, bw::2]
    return t


def unpack_s2d(g_t):
    """[n, 115, 115, 16] -> [n, 3, 224, 224]: y = 2 py - 4 + dy, x = 2 px - 4 + dx; border rows / columns and pad channels dropped."""
    n = g_t.shape[0]
    out = torch.zeros((n, 3, 224, 224), dtype=g_t.dtype)
    for y in range(224):
        py, dy = (y + 4) // 2, y % 2
        for dx in range(2):
            for c in range(3):
                # x = 2 px - 4 + dx for px = 2..113
                out[:, c, y, dx::2] = g_t[:, py, 2:114, s2d_channel(dy, dx, c)]
    return out


def operand_from_7x7(w7):
    """conv1 [64, 3, 7, 7] -> the forward operand [64, 256], K index r * 64 + s * 16 + k (fold.hip, K_CONV1_S2D): tap (r7, s7) =
    (2 r + dy - 1, 2 s + dx - 1); the entries of r7 < 0 or s7 < 0 and the pad channels are zero."""
    w = torch.zeros((64, 4, 4, 16), dtype=w7.dtype)
    for r in range(4):
        for dy in range(2):
            for s in range(4):
                for dx in range(2):
                    r7, s7 = 2 * r + dy - 1, 2 * s + dx - 1
                    if r7 >= 0 and s7 >= 0:
                        for c in range(3):
                            w[:, r, s, s2d_channel(dy, dx, c)] = w7[:, c, r7, s7]
    return w.reshape(64, 256)


def w7_from_operand(w):
    """The inverse of operand_from_7x7 on the entries that exist."""
    w = w.reshape(64, 4, 4, 16)
    w7 = torch.zeros((64, 3, 7, 7), dtype=w.dtype)
    for r in range(4):
        for dy in range(2):
            for s in range(4):
                for dx in range(2):
                    r7, s7 = 2 * r + dy - 1, 2 * s + dx - 1
                    if r7 >= 0 and s7 >= 0:
                        for c in range(3):
                            w7[:, c, r7, s7] = w[:, r, s, s2d_channel(dy, dx, c)]
    return w7


def valid_codes(oh, ow):
    """The arg-max codes (kh * 3 + kw of the 3 x 3 / stride 2 / pad 1 window) whose target (2 oh - 1 + kh, 2 ow - 1 + kw) lies
    inside 112 x 112."""
    return [kh * 3 + kw for kh in range(3) for kw in range(3) if 0 <= 2 * oh - 1 + kh < 112 and 0 <= 2 * ow - 1 + kw < 112]


def random_codes(rng, n):
    """uint8 [n, 56, 56, 64]: uniformly random valid codes."""
    kh = rng.integers(0, 3, size=(n, 56, 56, 64))
    kw = rng.integers(0, 3, size=(n, 56, 56, 64))
    kh[:, 0] = np.maximum(kh[:, 0], 1)
    kw[:, :, 0] = np.maximum(kw[:, :, 0], 1)
    return torch.from_numpy((kh * 3 + kw).astype(np.uint8))


def maxpool_bwd(g_pool, idx, round_bf16=True):
    """g_pool [n, 56, 56, 64] (float), idx uint8 -> g_c1 [n, 112, 112, 64] f32: every pixel the f32 sum of the <= 4 windows whose
    arg-max it is, in pooled-row then window-column order (maxpool_bwd_rows_kernel), rounded once to bf16 when asked."""
    n = g_pool.shape[0]
    g = g_pool.float()
    out = torch.zeros((n, 113, 113, 64), dtype=torch.float32)  # index = pixel + 1 (row / column -1 takes what a valid code never sends)
    # for a fixed pixel, the pooled row grows as kh falls and the window column grows as kw falls
    for kh in (2, 1, 0):
        for kw in (2, 1, 0):
            sel = torch.where(idx == kh * 3 + kw, g, torch.zeros_like(g))
            out[:, kh:kh + 112:2, kw:kw + 112:2] += sel
    assert float(out[:, 0].abs().max()) == 0.0 and float(out[:, :, 0].abs().max()) == 0.0, "a code points outside the image"
    out = out[:, 1:, 1:].contiguous()
    return out.to(torch.bfloat16).float() if round_bf16 else out


def input_grad_packed(g_c1, w):
    """g_c1 [n, 112, 112, 64], w [64, 256] (both float64 for the exact sum) -> [n, 3, 224, 224]:
    g_t[py][px][k] = sum_{r, s, co} g_c1[py - r][px - s][co] * w[co][r * 64 + s * 16 + k], unpacked."""
    n = g_c1.shape[0]
    prod = (g_c1.reshape(-1, 64) @ w).reshape(n, 112, 112, 4, 4, 16)  # [.., r, s, k]: the sum over co of every tap
    g_t = torch.zeros((n, 115, 115, 16), dtype=g_c1.dtype)
    for r in range(4):
        for s in range(4):
            g_t[:, r:r + 112, s:s + 112] += prod[:, :, :, r, s]
    return unpack_s2d(g_t)


def input_grad_conv_transpose(g_c1, w7):
    """The same through torch: conv_transpose2d of the NCHW gradient with the 7 x 7 weights, stride 2, padding 3, output_padding 1."""
    return F.conv_transpose2d(g_c1.permute(0, 3, 1, 2), w7, stride=2, padding=3, output_padding=1)


def stem_input_grad(g_pool, idx, w, round_bf16=True):
    """The operator: float64 sum over the (optionally bf16-rounded) max-pool backward tiles."""
    return input_grad_packed(maxpool_bwd(g_pool, idx, round_bf16).double(), w.double().reshape(64, 256))
