"""Beam decode attention alone at the 410M decode shape (B = 32 samples, H = 16, D = 64, 256 + 32 prefix keys, step t = 5) for
k = 1, 3, 5 beams: time per launch and the algorithmic bytes (prefix K/V once per sample + the beams' generated rows).  Under
``rocprofv3 --pmc FETCH_SIZE`` (a run of its own) the fabric bytes per launch show whether the prefix is read once whatever k is:
k = 1 / 3 / 5 launch attn_decode_beam_kernel<bf16, 64, 2 / 4 / 8>, three distinct kernel names (GPU box)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mafed_amd import ops  # noqa: E402

B, H, D, P, T, CAP, t = 32, 16, 64, 256, 32, 10, 5
S0, n, rot = P + T, 3 * H * D, D // 4
inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
ang = torch.arange(S0 + CAP, dtype=torch.float32)[:, None] * inv[None, :]
cos, sin = ang.cos().contiguous().cuda(), ang.sin().contiguous().cuda()
g = torch.Generator().manual_seed(0)
prefix = torch.randn(B * S0, n, generator=g).to(torch.bfloat16).cuda()
am = torch.ones(B, T, dtype=torch.int64).cuda()
for k in (1, 3, 5):
    new = torch.randn(B * k, CAP, n, generator=g).to(torch.bfloat16).cuda()
    anc = torch.tensor([[b * k + (r + j) % k for j in range(CAP)] for b in range(B) for r in range(k)], dtype=torch.int32).cuda()
    for _ in range(3):
        ops.attn_decode_beam(prefix, S0, new, t, B, k, anc, H, D, rot, cos, sin, am)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        ops.attn_decode_beam(prefix, S0, new, t, B, k, anc, H, D, rot, cos, sin, am)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    alg = (B * S0 * 2 * H * D + B * k * (t + 1) * 2 * H * D) * 2.0
    print(f"k={k}: {us:.1f} us per launch, algorithmic K/V read {alg / 1e6:.2f} MB ({alg / us / 1e6:.2f} TB/s)", flush=True)
