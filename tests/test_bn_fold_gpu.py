"""BatchNorm's finalize / params steps folded into the apply / dx kernels (csrc/batch_norm.hip, round 6: BnFin / BnBwdFin) against
the separate launches they replace (OGC_BN_FOLD=0): every output — activations, mean, rstd, running statistics, input gradient,
dgamma, dbeta, for the plain and the max-pooled form — must have the SAME BITS (each workgroup evaluates the same double-precision
expressions the one-thread-per-channel kernels did).  Three shapes: the writer workgroup alone in its row, one of two chunks
of a split row, and one of a halved row grid; the last two also with the statistics supplied in three partial sums.
The switch is read once per process: two child processes."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, torch
import ogc_amd
from ogc_amd import pointnet2_cuda as nat
g = torch.Generator().manual_seed(31)
out = {}


def run(tag, b, c, p, s, x, gamma, beta, gy, gout, slots=0):
    hw = p * s
    for relu in (0, 1):
        rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        y, mean, rstd = torch.empty_like(x), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        ws = torch.zeros(4 * c, dtype=torch.float64, device="cuda")
        nat.batch_norm_fwd_wrapper(b, c, hw, 1e-5, relu, 1, 0.1, x, gamma, beta, rm, rv, y, mean, rstd, ws, None, 0)
        gx, gg, gb = torch.empty_like(x), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        nat.batch_norm_bwd_wrapper(b, c, hw, relu, 1, x, gamma, beta, mean, rstd, gy, gx, gg, gb, ws)
        o, arg = torch.empty(b, c, p, device="cuda"), torch.empty(b, c, p, dtype=torch.int32, device="cuda")
        m2, r2 = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        nat.batch_norm_maxpool_fwd_wrapper(b, c, p, s, 1e-5, relu, 1, 0.1, x, gamma, beta, rm, rv, o, arg, m2, r2, ws, None, 0)
        px, pg, pb = torch.empty_like(x), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        nat.batch_norm_maxpool_bwd_wrapper(b, c, p, s, relu, 1, x, gamma, m2, r2, o, arg, gout, px, pg, pb, ws)
        res = dict(y=y, mean=mean, rstd=rstd, gx=gx, gg=gg, gb=gb, o=o, arg=arg, m2=m2, r2=r2, px=px, pg=pg, pb=pb, rm=rm, rv=rv)
        if slots:   # the statistics supplied in `slots` partial sums: the slot loops of bn_fin and of bn_finalize_kernel
            parts = x.double().permute(1, 0, 2, 3).reshape(c, -1).tensor_split(slots, dim=1)
            stats = torch.stack([torch.stack([t.sum(1), (t * t).sum(1)], 1) for t in parts]).contiguous()
            sm, sv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
            y3, m3, r3 = torch.empty_like(x), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
            nat.batch_norm_fwd_wrapper(b, c, hw, 1e-5, relu, 1, 0.1, x, gamma, beta, sm, sv, y3, m3, r3, None, stats, slots)
            o3, a3 = torch.empty_like(o), torch.empty_like(arg)
            m4, r4 = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
            nat.batch_norm_maxpool_fwd_wrapper(b, c, p, s, 1e-5, relu, 1, 0.1, x, gamma, beta, sm, sv, o3, a3, m4, r4, None, stats, slots)
            res.update(y3=y3, m3=m3, r3=r3, o3=o3, a3=a3, m4=m4, r4=r4, sm=sm, sv=sv)
        for k, v in res.items():
            out["%s%s_relu%d" % (tag, k, relu)] = v.cpu()


b, c, p, s = 3, 40, 300, 16
run("", b, c, p, s, (torch.randn(b, c, p, s, generator=g) * 2 + 0.3).cuda(), (torch.rand(c, generator=g) + 0.5).cuda(),
    torch.randn(c, generator=g).cuda(), torch.randn(b, c, p, s, generator=g).cuda(), torch.randn(b, c, p, generator=g).cuda())
# a plain shape whose statistics are split over two workgroups per row (hw = 8192) and a pooled shape whose row grid is halved
# (5 -> 3 workgroups per row): the writer workgroup is one of many.  Values on a lattice (x in eighths, gradients in sixteenths):
# their sums are exact, so the order of the atomics cannot differ between the two processes.
for tag, (b, c, p, s) in (("chunked_", (1, 2, 2048, 4)), ("halved_", (2, 1024, 300, 16))):
    x = (torch.randint(-255, 256, (b, c, p, s), generator=g).float() / 8).cuda()
    gamma = (torch.rand(c, generator=g) + 0.5) * (1 - 2 * (torch.arange(c) % 5 == 4).float())
    run(tag, b, c, p, s, x, gamma.cuda(), torch.randn(c, generator=g).cuda(),
        (torch.randint(1, 33, (b, c, p, s), generator=g).float() / 16).cuda(),
        (torch.randint(1, 33, (b, c, p), generator=g).float() / 16).cuda(), slots=3)
torch.save(out, sys.argv[1])
"""


def test_folded_batch_norm_has_the_bits_of_the_separate_launches(tmp_path):
    res = []
    for flag in ("1", "0"):
        path = str(tmp_path / ("bn_%s.pt" % flag))
        env = dict(os.environ, OGC_BN_FOLD=flag, PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", CHILD, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res.append(torch.load(path))
    assert set(res[0]) == set(res[1]) and len(res[0]) == 30 + 2 * 48
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
