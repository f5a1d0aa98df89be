"""Decided inputs and float64 references for the two kernel families of the MaskFormer head — csrc/small_linear.hip
(ogc_small_linear_fwd / _bwd) and csrc/attention.hip (ogc_attention_fwd / _bwd) — for tests/test_head_truth_gpu.py.  Host side:
numpy for the inputs and the conditions, torch float64 for the truth, torch float32 for the yardstick; no GPU needed, the library
is not imported.  The twin of tests/soft_corr_cases.py.

small_linear — EXACT.  x, W, dy and the bias are drawn from +-{1..8}/4 (no zeros: every term counts).  Every product is a multiple
of 1/16 of size at most 4, so a sum of up to 4096 of them stays below 2^14 in units of 2^-4: exact in fp32 in ANY order, with or
without fused multiply-adds.  y, dx, dW and db must therefore EQUAL the float64 result, and a dropped or doubled term moves a sum
by at least 1/16.  lin_make() asserts that torch's fp32 products on the host equal float64: the inputs are decided.

attention — float64 truth on decided inputs, for a case (B, H, D, Lq, Lk, layout):
  * K multiples of 1/4 in [-1, 1], V multiples of 1/4 in [-2, 2], dO standard normal;
  * query rows with q % 3 == 0 are FLAT (multiples of 1/4 in [-1, 1]: every key carries weight of order 1 / Lk), the others
    SHARP (multiples of 1/4 in [-4, 4]: a handful of keys carry the row);
  * D = 16: scale = 1/4, every score is a sum of 16 multiples of 1/64 below 16 — exact in fp32 in any order, scaled before or
    after (asserted).  D = 32 keeps the rounding of 32**-0.5;
  * the generator is seeded from the shape.
The truth is the op sequence softmax(scale * Q K^T) V and its autograd in torch float64 on the host; the same sequence in float32
on the host is the yardstick.  The gate of a tensor (out, prob, dq, dk, dv) and row class is test_group_norm_truth_gpu.Table's:
max(4 * err_torch32, 8 * 2**-24 * max|truth|); out, prob and dq are gated per row class (their probabilities differ by up to Lk).

att_make() asserts, in float64 and against the gate of the tensor that moves (COVER = 32, as in soft_corr_cases / seg_loss_cases);
each minimum runs over every sample, head and left-out index:
  forward  leaving any one key out of the softmax of flat row 0 moves `out` of that row by >= COVER x gate(out, flat)   (Lk > 1)
  dv       leaving any one query out of dV = sum_q P_qn dO_q moves it by >= COVER x gate(dv)
  dk       leaving any one query out of dK = scale sum_q dS_qn Q_q moves it by >= COVER x gate(dk)                     (Lk > 1)
  dq       leaving any one key out of dQ_q = scale sum_n dS_qn K_n over the flat rows moves one by >= COVER x gate(dq, flat);
           asserted only where Lq >= 10: with fewer flat rows a key can be light in all of them, and the forward and dk conditions,
           which read the same dS, stand in.
At Lk = 1 the truth of dq and dk is identically zero (dS = P (dP - dP) = 0), the gate is zero, and so must the kernel's output be.
"""
import collections
import functools

import numpy as np
import torch

U = 2.0 ** -24
COVER = 32.0

# ---- small_linear -----------------------------------------------------------------------------------------------------------------
SL_T, SL_K = 32, 64                    # tile edge, depth of a staged slice (csrc/small_linear.hip)
Lin = collections.namedtuple("Lin", "r ni no")
LIN_BASE = Lin(33, 65, 33)
LIN_R = (1, 31, 32, 33, 65, 160, 1024)
LIN_NI = (1, 63, 64, 65, 128, 129)
LIN_NO = (1, 31, 32, 33, 130, 384)
LIN_EXTRA = [Lin(1, 1, 1),             # one output, one term
             Lin(160, 128, 128),       # the model's projections and feed-forward layers
             Lin(160, 128, 384),       # the packed self-attention projection
             Lin(1024, 129, 33)]       # the last row count of the route, a slice of one column, a tile of one output column


def _unique(cases):
    return list(dict.fromkeys(cases))


LIN_CASES = _unique([LIN_BASE._replace(r=r) for r in LIN_R] + [LIN_BASE._replace(ni=n) for n in LIN_NI] +
                    [LIN_BASE._replace(no=n) for n in LIN_NO] + LIN_EXTRA)
LIN_SUBSET_CASES = [LIN_BASE, Lin(1, 65, 33), Lin(33, 129, 33)]      # all seven non-empty subsets of (dx, dW, db)
LIN_PACKED_CASES = [LIN_BASE, Lin(160, 128, 128)]                    # W[:no] of (3 no, ni), gw[:no] / gb[:no] of packed buffers


def lin_id(c):
    return "lin-%dx%dx%d" % c


def divup(a, b):
    return -(-a // b)


def lin_launch(r, ni, no, dx=True, dw=True, db=True):
    """The launches of ogc_small_linear_fwd / _bwd: tiles of 32 x 32 outputs, operands staged in slices 64 deep."""
    g = dict(fwd_tiles=divup(r, SL_T) * divup(no, SL_T), fwd_slices=divup(ni, SL_K), fwd_last=ni - (divup(ni, SL_K) - 1) * SL_K)
    g["dx_tiles"] = divup(r, SL_T) * divup(ni, SL_T) if dx else 0                  # reduce over no
    g["dx_slices"] = divup(no, SL_K)
    g["dw_tiles"] = divup(no, SL_T) * divup(ni, SL_T) if (dw or db) else 0         # reduce over r
    g["dw_slices"] = divup(r, SL_K)
    g["db_tiles"] = divup(no, SL_T) if db else 0                                   # the dW tiles of column block 0
    g["zero_columns"] = bool(db and not dw)                                        # frozen weight: the tiles write no dW
    g["edge"] = (r % SL_T, ni % SL_T, no % SL_T)
    return g


def _lattice(rng, shape):
    return (rng.integers(1, 9, shape) * rng.choice([-1, 1], shape) / 4.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lin_make(c, seed=0):
    """dict of fp32 numpy arrays: x (r, ni), w (no, ni), b (no,), dy (r, no) and the exact y (with bias), y0 (without), dx, dw, db."""
    rng = np.random.default_rng([seed, c.r, c.ni, c.no, 51])
    d = dict(x=_lattice(rng, (c.r, c.ni)), w=_lattice(rng, (c.no, c.ni)), b=_lattice(rng, (c.no,)), dy=_lattice(rng, (c.r, c.no)))
    for a in (d["x"], d["w"], d["b"], d["dy"]):
        assert bool((np.abs(a) >= 0.25).all() and (np.abs(a) <= 2).all() and (a * 4 == np.rint(a * 4)).all())
    x, w, b, dy = (d[k].astype(np.float64) for k in ("x", "w", "b", "dy"))
    want = dict(y0=x @ w.T, y=x @ w.T + b, dx=dy @ w, dw=dy.T @ x, db=dy.sum(0))
    # decided: torch's own fp32 products on the host give the float64 result, bit for bit
    t = {k: torch.from_numpy(d[k]) for k in ("x", "w", "b", "dy")}
    got = dict(y0=torch.nn.functional.linear(t["x"], t["w"]), y=torch.nn.functional.linear(t["x"], t["w"], t["b"]),
               dx=t["dy"] @ t["w"], dw=t["dy"].t() @ t["x"], db=t["dy"].sum(0))
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and np.array_equal(got[k].numpy().astype(np.float64), v), (lin_id(c), k)
        assert float(np.abs(v).max()) * 16 < 2 ** 24 and bool((v * 16 == np.rint(v * 16)).all())
        d[k] = v.astype(np.float32)
    return d


# ---- attention --------------------------------------------------------------------------------------------------------------------
AT_THREADS, AT_WAVE, AT_LDS = 256, 64, 64 * 1024          # csrc/attention.hip
LAYOUTS = ("cross", "self", "padded")
Att = collections.namedtuple("Att", "B H D Lq Lk layout")


def att(B, H, D, Lq, Lk, layout="cross"):
    assert layout in LAYOUTS and (layout != "self" or Lq == Lk)
    return Att(B, H, D, Lq, Lk, layout)


def att_id(c):
    return "att-%dx%dx%d-%dx%d-%s" % c


ATT_LK = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 991)
ATT_LQ = (1, 3, 4, 5, 8, 9, 16, 17, 257)

# forward: one wavefront per (sample, head, query), four per workgroup, lane l takes keys l, l + 64, ...
# backward: one workgroup of 256 per (sample, head): a thread per key (stride 256), dsum with stride 256 over the queries, the
# lq * D loops with stride 256, dQ four keys at a time with a tail; LDS 4 * (2 lq D + round4(lq) + lq lk) bytes <= 64 KiB
ATT_CASES = [
    att(1, 1, 16, 1, 1),                  # ONE item: three idle wavefronts; Lk = 1: 63 idle lanes, dq and dk exactly zero
    att(1, 2, 32, 3, 2),                  # two keys: the dQ tail alone, twice; items = 6: two idle wavefronts
    att(1, 2, 16, 4, 3, "padded"),        # dQ: a tail of three and no quad
    att(3, 1, 16, 5, 4),                  # dQ: one quad and no tail; items = 15; B = 3
    att(1, 2, 32, 5, 5, "self"),          # dQ: one quad and a tail of one; self-attention at D = 32
    att(1, 2, 16, 3, 5, "padded"),        # Lq = 3: one flat row, two sharp
    att(1, 8, 16, 1, 63),                 # Lq = 1: the flat class alone; one idle lane; H = 8
    att(1, 2, 32, 8, 64, "padded"),       # every lane one key; lq * D = 256 at D = 32: one full pass of the lq * D loops
    att(3, 2, 16, 9, 65),                 # lane 0 takes a second key; the memory-contract case
    att(1, 2, 32, 9, 65, "padded"),       # lq * D = 288 at D = 32: a second pass of 32
    att(1, 2, 32, 5, 63),                 # lq * D = 160 at D = 32: below one pass
    att(1, 2, 16, 16, 127),               # lq * D = 256 at D = 16
    att(1, 1, 32, 16, 128),               # two keys on every lane; H = 1 at D = 32
    att(3, 8, 16, 17, 129),               # lq * D = 272 at D = 16: a second pass of 16; three keys on lane 0; B = 3 with H = 8
    att(1, 2, 16, 9, 255, "padded"),      # lq * D = 144 at D = 16; the backward's key loop one thread short of full
    att(1, 2, 32, 4, 256),                # every thread of the backward one key
    att(1, 2, 16, 5, 257),                # thread 0 takes a second key (stride 256)
    att(3, 2, 32, 3, 257),                # the same at D = 32, one flat row (the dq condition is not asked for); items = 18
    att(1, 2, 32, 8, 255),                # the same key loop at D = 32 with lq * D = 256: both loops within one pass
    att(1, 1, 32, 5, 991),                # 15 keys on most lanes, 16 on lanes 0 .. 30, at D = 32
    att(1, 1, 16, 16, 991),               # LDS = 65536 bytes exactly: the largest backward there is at lq = 16
    att(1, 8, 16, 10, 1500),              # beyond the model's 512 keys: 24 keys on lanes 0 .. 27; six passes of the key loop
    att(1, 1, 16, 257, 5),                # Lq = 257: dsum's second pass holds one query; 4112 elements in the lq * D loops
    att(1, 2, 16, 257, 3),                # the same with two heads and the dQ tail alone
    att(1, 2, 16, 17, 17, "self"),        # self-attention, thirds of one packed tensor, D = 16
    att(3, 2, 32, 17, 17, "self"),        # the memory-contract case of the self layout
    att(1, 1, 16, 64, 64, "self"),        # self-attention with a full wavefront of keys; items = 64
    att(1, 8, 16, 10, 512),               # the model's cross-attention (one sample)
    att(3, 8, 16, 10, 10, "self"),        # the model's self-attention among the slots
]
CONTRACT_CASES = [att(3, 2, 16, 9, 65), att(3, 2, 32, 17, 17, "self")]
LIMIT_CASE = att(1, 1, 16, 16, 991)                    # exactly 64 KiB: through the wrappers only
GATE_LIMIT = (16, 990, 16)                             # the largest lk the Python gate admits at lq = 16: through the module
OVER_CASE = att(1, 1, 16, 16, 992)                     # the backward is refused; the forward runs (not in ATT_CASES)


def att_lds(lq, lk, d):
    """attn_bwd_lds of csrc/attention.hip, in bytes."""
    return 4 * (2 * lq * d + (lq + 3) // 4 * 4 + lq * lk)


def att_fwd_launch(B, H, Lq, Lk):
    items = B * H * Lq
    blocks = divup(items, AT_THREADS // AT_WAVE)
    share = [len(range(lane, Lk, AT_WAVE)) for lane in range(AT_WAVE)]
    return dict(items=items, blocks=blocks, idle_waves=blocks * (AT_THREADS // AT_WAVE) - items, share=share,
                idle_lanes=share.count(0), steps=max(share), ragged=len(set(share)) > 1)


def att_bwd_launch(B, H, D, Lq, Lk):
    return dict(blocks=B * H, key_passes=divup(Lk, AT_THREADS), key_last=Lk - (divup(Lk, AT_THREADS) - 1) * AT_THREADS,
                dsum_passes=divup(Lq, AT_THREADS), ld_passes=divup(Lq * D, AT_THREADS), ld_tail=(Lq * D) % AT_THREADS,
                quads=Lk // 4, tail=Lk % 4, lds=att_lds(Lq, Lk, D))


def flat_rows(Lq):
    r = np.zeros(Lq, bool)
    r[0::3] = True
    return r


def att_scale(D):
    return 0.25 if D == 16 else D ** -0.5


def _heads(a, H):
    """(B, L, E) -> (B, H, L, D)"""
    B, L, E = a.shape
    return a.reshape(B, L, H, E // H).transpose(0, 2, 1, 3)


@functools.lru_cache(maxsize=None)
def att_inputs(c):
    """dict of fp32 numpy arrays q, do (B, Lq, E) and k, v (B, Lk, E), E = H * D."""
    rng = np.random.default_rng([c.B, c.H, c.D, c.Lq, c.Lk, LAYOUTS.index(c.layout), 41])
    E = c.H * c.D
    flat = flat_rows(c.Lq)
    q = rng.integers(-16, 17, (c.B, c.Lq, E))
    q[:, flat] = rng.integers(-4, 5, (c.B, int(flat.sum()), E))
    d = dict(q=(q / 4.0).astype(np.float32), k=(rng.integers(-4, 5, (c.B, c.Lk, E)) / 4.0).astype(np.float32),
             v=(rng.integers(-8, 9, (c.B, c.Lk, E)) / 4.0).astype(np.float32),
             do=rng.standard_normal((c.B, c.Lq, E)).astype(np.float32))
    assert float(np.abs(d["q"][:, flat]).max()) <= 1 and float(np.abs(d["q"]).max()) <= 4
    assert float(np.abs(d["k"]).max()) <= 1 and float(np.abs(d["v"]).max()) <= 2
    if c.D == 16:
        # every score exact in fp32: scaled first (the kernel) or last (the op sequence), summed forwards or backwards
        qh, kh = _heads(d["q"], c.H), _heads(d["k"], c.H)
        want = 0.25 * np.einsum("bhqd,bhnd->bhqn", qh.astype(np.float64), kh.astype(np.float64))
        for pre in (np.float32(0.25), np.float32(1)):
            terms = (qh * pre)[:, :, :, None, :] * kh[:, :, None, :, :]
            assert terms.dtype == np.float32
            for t in (terms, terms[..., ::-1]):
                s = np.cumsum(t, axis=-1, dtype=np.float32)[..., -1] * (np.float32(0.25) / pre)
                assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), want), att_id(c)
    return d


def att_reference(c, d, dtype):
    """softmax(scale * Q K^T) V per head and its autograd in torch `dtype` on the host -> out, prob, dq, dk, dv."""
    q, k, v = (torch.from_numpy(d[key]).to(dtype).requires_grad_(True) for key in ("q", "k", "v"))
    do = torch.from_numpy(d["do"]).to(dtype)
    B, H, D, Lq, Lk = c.B, c.H, c.D, c.Lq, c.Lk
    qh, kh, vh = (t.view(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    prob = torch.softmax(att_scale(D) * (qh @ kh.transpose(2, 3)), -1)
    out = (prob @ vh).transpose(1, 2).reshape(B, Lq, H * D)
    dq, dk, dv = torch.autograd.grad((out * do).sum(), [q, k, v])
    return dict(out=out.detach(), prob=prob.detach(), dq=dq, dk=dk, dv=dv)


TENSORS = ("out", "prob", "dq", "dk", "dv")


def att_parts(c, name, t):
    """[(label, the part of tensor `name` gated on its own)]: out, prob and dq per row class, dk and dv whole."""
    if name in ("dk", "dv"):
        return [(name, t)]
    flat = torch.from_numpy(flat_rows(c.Lq))
    parts = [(name + " flat", t[:, :, flat] if name == "prob" else t[:, flat])]
    if c.Lq > 1:
        parts.append((name + " sharp", t[:, :, ~flat] if name == "prob" else t[:, ~flat]))
    return parts


def att_gates(c, truth, yard):
    """{label: (gate, err_torch32)} — Table's max-abs gate of every gated part, from the host yardstick."""
    gates = {}
    for name in TENSORS:
        for (label, t), (_, y) in zip(att_parts(c, name, truth[name]), att_parts(c, name, yard[name])):
            err = float((y.double() - t).abs().max()) if t.numel() else 0.0
            gates[label] = (max(4 * err, 8 * U * float(t.abs().max())), err)
    return gates


@functools.lru_cache(maxsize=None)
def att_make(c):
    """att_inputs(c) and: truth (float64), yard (float32), gates, and the measured conditions fwd / dv / dk / dq (smallest movement
    in units of the gate; absent where the condition has nothing to ask)."""
    d = dict(att_inputs(c))
    d["truth"], d["yard"] = att_reference(c, d, torch.float64), att_reference(c, d, torch.float32)
    d["gates"] = att_gates(c, d["truth"], d["yard"])
    H, Lq, Lk, scale = c.H, c.Lq, c.Lk, att_scale(c.D)
    flat = flat_rows(Lq)
    qh, kh, vh, doh = (_heads(d[key].astype(np.float64), H) for key in ("q", "k", "v", "do"))
    s = scale * np.einsum("bhqd,bhnd->bhqn", qh, kh)
    e = np.exp(s - s.max(-1, keepdims=True))
    P = e / e.sum(-1, keepdims=True)
    O = P @ vh
    dP = np.einsum("bhqd,bhnd->bhqn", doh, vh)
    dS = P * (dP - (P * dP).sum(-1, keepdims=True))
    # the closed forms are the truth (an independent route to it)
    for name, mine in (("prob", P), ("out", O.transpose(0, 2, 1, 3).reshape(c.B, Lq, -1)),
                       ("dv", np.einsum("bhqn,bhqd->bhnd", P, doh).transpose(0, 2, 1, 3).reshape(c.B, Lk, -1)),
                       ("dk", scale * np.einsum("bhqn,bhqd->bhnd", dS, qh).transpose(0, 2, 1, 3).reshape(c.B, Lk, -1)),
                       ("dq", scale * np.einsum("bhqn,bhnd->bhqd", dS, kh).transpose(0, 2, 1, 3).reshape(c.B, Lq, -1))):
        t = d["truth"][name].numpy()
        assert float(np.abs(mine - t).max()) <= 1e-12 * max(float(np.abs(t).max()), 1.0), (att_id(c), name)
    if Lk == 1:
        assert not d["truth"]["dq"].any() and not d["truth"]["dk"].any() and not d["yard"]["dq"].any() and not d["yard"]["dk"].any()
        assert d["gates"]["dq flat"][0] == 0 and d["gates"]["dk"][0] == 0
    if Lk > 1:
        p0 = P[:, :, 0, :]                                                                   # (B, H, Lk): flat row 0
        move = p0 / (1 - p0) * np.abs(O[:, :, 0, None, :] - vh).max(-1)                      # out' - out, key n left out
        d["fwd"] = float(move.min() / d["gates"]["out flat"][0])
        assert d["fwd"] >= COVER, (att_id(c), "fwd", d["fwd"])
    d["dv_cover"] = float((P.max(-1) * np.abs(doh).max(-1)).min() / d["gates"]["dv"][0])       # query q left out of dV
    assert d["dv_cover"] >= COVER, (att_id(c), "dv", d["dv_cover"])
    if Lk > 1:
        d["dk_cover"] = float((scale * np.abs(dS).max(-1) * np.abs(qh).max(-1)).min() / d["gates"]["dk"][0])
        assert d["dk_cover"] >= COVER, (att_id(c), "dk", d["dk_cover"])
        move = scale * np.abs(dS[:, :, flat]).max(2) * np.abs(kh).max(-1)                    # (B, H, Lk): key n left out of dQ
        d["dq_cover"] = float(move.min() / d["gates"]["dq flat"][0])
        if Lq >= 10:
            assert d["dq_cover"] >= COVER, (att_id(c), "dq", d["dq_cover"])
    return d


def gate_admits(lq, lk, d):
    """The LDS clause of fused.attention_core_available, written out (the test holds the function itself against it)."""
    return 4 * (lq * lk + 2 * lq * d + lq + 4) <= AT_LDS
