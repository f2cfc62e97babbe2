"""``ext().rope_kv_write_chunk`` (RoPE + paged K/V write of a packed chunk pass) on the GPU: bit for bit against the
one-token kernel ``ext().rope_kv_append_paged`` called with one row per token, against float64 math, and its error
tokens.  Three segments of 37, 0 and 70 tokens starting at 0, 5 and 2 * page - 3: an empty one, one crossing two page
boundaries from a mid-page start; shuffled, interleaved page ids; a sentinel in every pool byte."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops._ext import ext  # noqa: E402
from scaling_amd.ops.rope import rope_kv_write_chunk, rope_tables  # noqa: E402

DEV = torch.device("cuda", 0)
MAX_PAGES, NUM_PAGES, LENS = 6, 24, (37, 0, 70)


def _run(pool, interleaved, frac, hd, page, nq, nkv, starts=None, edit_table=None, inf_at=None, sentinel=7.0,
         lens=LENS, max_pages=MAX_PAGES):
    """The chunk kernel and the one-token oracle on the same inputs: (q, k pool, v pool, k scales, v scales, err) of
    each, the tokens' positions and segments, the table and x."""
    g = torch.Generator().manual_seed(hd + page + nq)
    dtype = torch.float16 if pool == "fp16" else torch.bfloat16
    rd = int(hd * frac)
    starts = (0, 5, 2 * page - 3) if starts is None else starts
    num_pages = 4 * max_pages
    cos, sin = rope_tables(rd, max_pages * page + 64, 10000.0, interleaved, dtype, DEV)
    perm = torch.randperm(num_pages, generator=g).to(torch.int32)
    table = torch.stack([perm[s::3][:max_pages] for s in range(3)])
    if edit_table is not None:
        table[edit_table[0], edit_table[1]] = edit_table[2]
    T = sum(lens)
    x = (2 * torch.randn(T, nq + 2 * nkv, hd, generator=g)).to(dtype)
    if inf_at is not None:
        x[inf_at[0], nq + inf_at[1], 3] = float("inf")
    seg = torch.repeat_interleave(torch.arange(3), torch.tensor(lens))
    cu = torch.tensor([0, lens[0], lens[0] + lens[1], T], dtype=torch.int32)
    pos = torch.tensor(starts)[seg] + torch.arange(T) - cu[seg]
    x, table_d = x.to(DEV), table.to(DEV)

    def pools():
        rows = num_pages * page
        if pool == "fp8":
            return [torch.full((rows, nkv, hd), 0x5A, dtype=torch.uint8, device=DEV) for _ in range(2)] + \
                   [torch.full((nkv, rows), 3.0, device=DEV) for _ in range(2)]
        return [torch.full((rows, nkv, hd), sentinel, dtype=dtype, device=DEV) for _ in range(2)] + [None, None]

    got, ref = pools(), pools()
    e_got, e_ref = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    q_got = rope_kv_write_chunk(x, cos, sin, cu.to(DEV), torch.tensor(starts, device=DEV), table_d, page, nq, nkv, rd,
                                interleaved, got[0], got[1], e_got, None if pool != "fp8" else (got[2], got[3]))
    q_ref = ext().rope_kv_append_paged(x, cos, sin, pos.to(DEV), nq, nkv, rd, interleaved, ref[0], ref[1], e_ref,
                                       table_d[seg.to(DEV)].contiguous(), page, ref[2], ref[3])
    return dict(got=[q_got] + got + [e_got], ref=[q_ref] + ref + [e_ref], pos=pos, seg=seg, table=table, x=x,
                cos=cos, sin=sin, rd=rd)


def _same_bits(r):
    for name, a, b in zip(("q", "k pool", "v pool", "k scale", "v scale", "err"), r["got"], r["ref"]):
        if a is not None:
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), name


@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 2), (3, 1)])
@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("frac", [1.0, 0.5])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("pool", ["bf16", "fp16", "fp8"])
def test_bitwise_against_the_one_token_kernel(pool, interleaved, frac, hd, page, nq, nkv):
    r = _run(pool, interleaved, frac, hd, page, nq, nkv)
    _same_bits(r)  # q, every pool byte (unowned rows keep the sentinel) and -- FP8 -- every scale
    assert r["got"][-1].item() == 0


@pytest.mark.parametrize("pool", ["bf16", "fp8"])
@pytest.mark.parametrize("nq,nkv,n,interleaved", [(3, 1, 6000, False), (3, 1, 9000, True), (8, 2, 9000, False)])
def test_bitwise_with_several_heads_per_workgroup(pool, nq, nkv, n, interleaved):
    """Passes long enough that the launcher gives a workgroup more than one head (the shapes above get one each).  At
    head dim 128 a workgroup holds 16 tokens, the grid T / 16 + 3 tiles and ceil(2048 / tiles) head slices: 12000 tokens
    -> 3 slices of 2 of the 5 heads {q0 q1} {q2 k0} {v0}; 18000 tokens -> 2 slices, of 3 of 5 heads {q0 q1 q2} {k0 v0}
    and of 6 of 12 heads {q0..q5} {q6 q7 k0 k1 v0 v1}: slices across the q | k and the k | v boundary, and short last
    slices."""
    r = _run(pool, interleaved, 1.0, 128, 64, nq, nkv, lens=(n, 0, n), max_pages=-(-(125 + n) // 64))
    _same_bits(r)
    assert r["got"][-1].item() == 0


@pytest.mark.parametrize("interleaved", [False, True])
def test_against_float64(interleaved):
    """q and the written k rows within 2^-8 (|x_a| + |x_b|) of the float64 rotation by the fp32 tables (x_a, x_b the
    rotation's two inputs: one bf16 rounding, 2^-9 relative, of an fp32 result of magnitude <= |x_a| + |x_b| that is
    itself a few fp32 ulps off); v rows are exact copies."""
    hd, page, nq, nkv = 64, 32, 8, 2
    r = _run("bf16", interleaved, 1.0, hd, page, nq, nkv)
    x, pos = r["x"].double().cpu(), r["pos"]
    c, s = r["cos"].double().cpu()[pos][:, None, :], r["sin"].double().cpu()[pos][:, None, :]
    xa, xb = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., : hd // 2], x[..., hd // 2 :])
    oa, ob, tol = xa * c - xb * s, xb * c + xa * s, 2.0 ** -8 * (xa.abs() + xb.abs())
    want = torch.stack([oa, ob], -1).flatten(-2) if interleaved else torch.cat([oa, ob], -1)
    tol = torch.stack([tol, tol], -1).flatten(-2) if interleaved else torch.cat([tol, tol], -1)
    rows = (r["table"][r["seg"], pos // page].long() * page + pos % page).to(DEV)
    got = torch.cat([r["got"][0], r["got"][1][rows]], 1).double().cpu()
    err = (got - want[:, : nq + nkv]).abs()
    print(f"max error / bound: {(err / tol[:, : nq + nkv].clamp_min(1e-30)).max().item():.3f}")
    assert (err <= tol[:, : nq + nkv]).all()
    assert torch.equal(r["got"][2][rows], r["x"][:, nq + nkv :])


@pytest.mark.parametrize("pool", ["bf16", "fp8"])
@pytest.mark.parametrize("case", ["past_the_pages", "entry_minus_one", "entry_2_30"])
def test_error_tokens(pool, case):
    """Exactly the error tokens get zero q rows and write nothing (pool rows outside the good tokens' keep their NaN
    sentinel); bit 0 of err is set; every other token is what the one-token kernel writes."""
    hd, page, nq, nkv = 64, 32, 8, 2
    kw = {"past_the_pages": dict(starts=(0, 5, MAX_PAGES * page - 68)), "entry_minus_one": dict(edit_table=(0, 0, -1)),
          "entry_2_30": dict(edit_table=(2, 2, 2 ** 30))}[case]
    r = _run(pool, False, 1.0, hd, page, nq, nkv, sentinel=float("nan"), **kw)
    pos, seg = r["pos"], r["seg"]
    entry = r["table"][seg, (pos // page).clamp(max=MAX_PAGES - 1)].long()
    bad = (pos >= MAX_PAGES * page) | (entry < 0) | (entry >= NUM_PAGES)
    assert bad.sum().item() == {"past_the_pages": 2, "entry_minus_one": 32, "entry_2_30": 32}[case]
    _same_bits(r)
    q = r["got"][0].cpu()
    assert (q[bad] == 0).all() and (q[~bad] != 0).flatten(1).any(1).all() and r["got"][-1].item() == 1
    untouched = torch.ones(NUM_PAGES * page, dtype=torch.bool)
    untouched[(entry * page + pos % page)[~bad]] = False
    k = r["got"][1].cpu()
    assert ((k[untouched] == 0x5A) if pool == "fp8" else k[untouched].isnan()).all()
    assert (r["got"][3].cpu()[:, untouched] == 3.0).all() if pool == "fp8" else True


def test_fp8_nonfinite_value_sets_bit_1():
    r = _run("fp8", True, 1.0, 64, 32, 8, 2, inf_at=(50, 1))
    _same_bits(r)
    assert r["got"][-1].item() == 2 and not ((r["got"][1] & 0x7F) == 0x7F).any()  # no NaN code (0x7f / 0xff)
