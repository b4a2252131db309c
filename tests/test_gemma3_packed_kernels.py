"""The kernels of om_gemma3_encoder_forward_packed, alone: grouped-query attention over heads of 256 columns walking PACKED sequences
(csrc/attention_d256.hip omk_attention_gqa_d256_packed) against the padded kernel bit for bit and against the float64 restatement
under the bound of tests/test_gemma3_kernels.py, and the q / k RMSNorm + rotary pass of Gemma3's form gathered through a row_map."""
import pytest
import torch

from openmatch_amd import native as N
from tests.test_attention_kernels import BF16, DEV, F16, F32, NAME, TORCH_DT, bits, mask_extent, new_ctx, pack_rows, rows_of, untouched
from tests.test_gemma3_kernels import D, SCALE, _hf_rotary, assert_case, grouped_inputs, launch, run_case

DTYPES = [F32, BF16, F16]
# the extents cross the wave edge (31 / 63 / 65), the 64-key chunk edge (63 / 64 / 65, 128 / 257) and the 128-query block edge (128 / 129,
# 257 / 300); the longest sequence fills the pitch, so band or full is decided on the same L by both launches
RAGGED = {129: [1, 63, 64, 65, 129], 640: [31, 128, 257, 300, 640]}


def right_padded(lengths, L):
    mask = torch.zeros(len(lengths), L, dtype=torch.int64)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    return mask


def launch_packed(dtype, qp, ctx, mask, cu, B, L, heads, kv, w=0, scale=SCALE):
    rc = N.lib().om_debug_attention_gqa_d256_packed(dtype, N.ptr(qp), N.ptr(ctx), N.ptr(mask), N.ptr(cu), B, L, heads, kv, scale, w, N.stream_ptr())
    torch.cuda.synchronize()
    return rc


def run_packed(dtype, qkv, mask, L, heads, kv, w, extra=7):
    """Packs the padded projection `qkv` [B * L, P] by the mask's extents, runs the packed kernel, returns (ctx incl. guard rows, src rows
    of the padded layout, token count).  The rows past the token count of the packed projection hold NaN: nothing may read them."""
    B = mask.shape[0]
    kmax = mask_extent(mask)
    total = int(kmax.sum())
    rows = total + extra
    cu, _, row_map = pack_rows(kmax, L, rows)
    src = row_map[:total].long()
    assert (row_map[total:] < 0).all()
    qp = torch.full((rows, qkv.shape[1]), float("nan"), dtype=TORCH_DT[dtype], device=DEV)
    qp[:total] = qkv[src]
    qp0 = qp.clone()
    ctx = new_ctx(rows, heads * D, dtype)
    assert launch_packed(dtype, qp, ctx, mask, cu, B, L, heads, kv, w) == 0, N.lib().om_last_error()
    assert torch.equal(bits(qp, dtype), bits(qp0, dtype)), "the packed projection was written"
    return ctx, src, total


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("heads,kv", [(3, 1), (4, 2)])
@pytest.mark.parametrize("w", [0, 1, 64, 256])
@pytest.mark.parametrize("L", sorted(RAGGED))
def test_packed_attention_d256_is_the_padded_kernel_row_for_row(L, w, heads, kv, dtype):
    """Ragged right-padded batches: every packed row up to each sequence's extent carries the bits of its padded row; rows of the packed
    ctx at and beyond cu[B] keep the fill pattern.  w = 256 at L = 129 reaches every key: both launches take the full kernel."""
    mask = right_padded(RAGGED[L], L).to(DEV)
    B = mask.shape[0]
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=3 + L + w)
    padded = new_ctx(B * L, heads * D, dtype)
    assert launch(dtype, qkv, padded, mask, B, L, heads, kv, w) == 0, N.lib().om_last_error()
    ctx, src, total = run_packed(dtype, qkv, mask, L, heads, kv, w)
    assert total == sum(RAGGED[L])
    assert torch.equal(bits(ctx[:total].contiguous(), dtype), bits(padded[:B * L][src].contiguous(), dtype))
    assert untouched(ctx[total:], dtype), "rows at and beyond the token count were written"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("w", [0, 256])
def test_packed_attention_d256_against_float64(w, dtype):
    """The packed kernel's rows, put back at their padded places, under the bound test_gemma3_kernels.py holds the padded kernel to: one
    full and one band case at L = 640"""
    L, heads, kv = 640, 3, 1
    mask = right_padded(RAGGED[L], L)
    padded, ref, bound, contract = run_case(dtype, L, heads, kv, w, mask=mask, tag="ragged")
    B = mask.shape[0]
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=91 + 13 * L + heads + kv)      # run_case's inputs
    ctx, src, total = run_packed(dtype, qkv, mask.to(DEV), L, heads, kv, w)
    got = padded.clone().reshape(B * L, heads * D)      # rows past an extent keep the padded kernel's values: no contract is lost
    got[src] = ctx[:total]
    assert_case(got.view(B, L, heads * D), ref, bound, contract, heads, f"d256 packed {NAME[dtype]} L={L} w={w}")
    inside = torch.zeros(B * L, dtype=torch.bool, device=DEV)
    inside[src] = True
    ratio = ((got.view(B, L, -1).double() - ref).abs() / bound)[rows_of(inside.view(B, L) & contract, heads * D)]
    assert ratio.numel() == total * heads * D and ratio.max().item() <= 1.0      # every packed row is under contract and inside the bound


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("w", [0, 40])
def test_masked_tokens_inside_an_extent_stay_masked(w, dtype):
    """Leading zeros: the extent runs to the last unmasked token, so the masked head of the sequence is packed with it and must stay
    hidden as a key -- the packed rows equal the padded kernel's, and rewriting K / V of the masked keys changes no unmasked query"""
    L, heads, kv = 200, 3, 1
    mask = torch.zeros(3, L, dtype=torch.int64)
    mask[0, :150] = 1
    mask[1, 30:170] = 1             # 30 leading zeros inside an extent of 170
    mask[2, 70:] = 1                # left-padded: extent L
    mask = mask.to(DEV)
    B = 3
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=17 + w)
    padded = new_ctx(B * L, heads * D, dtype)
    assert launch(dtype, qkv, padded, mask, B, L, heads, kv, w) == 0
    ctx, src, total = run_packed(dtype, qkv, mask, L, heads, kv, w)
    assert total == 150 + 170 + 200
    assert torch.equal(bits(ctx[:total].contiguous(), dtype), bits(padded[:B * L][src].contiguous(), dtype))
    keep = (mask.view(-1)[src] != 0)      # queries that are tokens (a masked query whose band holds no token averages masked keys)
    a = ctx[:total][keep].contiguous()
    q2 = qkv.clone().view(B, L, -1)
    other = grouped_inputs(dtype, B, L, heads, kv, seed=99).view(B, L, -1)
    hidden = (mask == 0)
    q2[:, :, heads * D:][hidden] = other[:, :, heads * D:][hidden]
    ctx2, _, _ = run_packed(dtype, q2.view(B * L, -1), mask, L, heads, kv, w)
    assert torch.equal(bits(ctx2[:total][keep].contiguous(), dtype), bits(a, dtype))
    assert torch.isfinite(ctx[:total].double()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("w", [0, 20])
def test_a_fully_masked_sequence_packs_at_full_extent_and_stays_finite(w, dtype):
    """omk_mask_extent gives a row without an unmasked key the extent L: it is packed whole, every key scores the finite masked value
    and the rows stay finite (the padded kernel's bits)"""
    L, heads, kv = 150, 3, 1
    mask = torch.ones(3, L, dtype=torch.int64)
    mask[0, 100:] = 0
    mask[1] = 0
    mask = mask.to(DEV)
    assert mask_extent(mask).tolist() == [100, L, L]
    qkv = grouped_inputs(dtype, 3, L, heads, kv, seed=23)
    padded = new_ctx(3 * L, heads * D, dtype)
    assert launch(dtype, qkv, padded, mask, 3, L, heads, kv, w) == 0
    ctx, src, total = run_packed(dtype, qkv, mask, L, heads, kv, w)
    assert total == 100 + 2 * L
    assert torch.isfinite(ctx[:total].double()).all()
    assert torch.equal(bits(ctx[:total].contiguous(), dtype), bits(padded[:3 * L][src].contiguous(), dtype))
    assert untouched(ctx[total:], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("kind", ["sliding", "full"])
def test_qknorm_rope_d256_rows_form_is_the_plain_form_row_for_row(kind, dtype):
    """packed rows: row t takes the position row_map[t] % L and equals the plain pass's row row_map[t]; rows with row_map < 0 are left
    alone"""
    L, heads, kv, eps = 129, 2, 1, 1e-6
    lengths = RAGGED[L]
    B = len(lengths)
    inv, scaling, _, _ = _hf_rotary(kind, L)
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(B * L, (heads + 2 * kv) * D, generator=g) * 1.7).to(TORCH_DT[dtype]).to(DEV)
    wq, wk = (1.0 + 0.3 * torch.randn(D, generator=g)).to(DEV), (1.0 + 0.3 * torch.randn(D, generator=g)).to(DEV)
    kmax = mask_extent(right_padded(lengths, L).to(DEV))
    total = int(kmax.sum())
    rows = total + 50
    _, _, row_map = pack_rows(kmax, L, rows)
    assert (row_map[total:] < 0).all()
    plain = x.clone()
    N.check(N.lib().om_debug_qknorm_rope_d256(dtype, N.ptr(plain), B * L, L, heads, kv, N.ptr(wq), N.ptr(wk), eps, inv, scaling, N.stream_ptr()))
    packed = torch.zeros(rows, x.shape[1], dtype=x.dtype, device=DEV)
    packed[:total] = x[row_map[:total].long()]
    packed[total:] = 3.0
    N.check(N.lib().om_debug_qknorm_rope_d256_rows(dtype, N.ptr(packed), rows, L, heads, kv, N.ptr(wq), N.ptr(wk), eps, inv, scaling,
                                                   N.ptr(row_map), N.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits(packed[:total].contiguous(), dtype), bits(plain[row_map[:total].long()].contiguous(), dtype))
    assert (packed[total:] == 3.0).all()
    assert not torch.equal(plain, x)
    # a row that is not its sequence's first takes its own column as position, not its packed row number
    assert int(row_map[lengths[0] + 5]) % L == 5 and lengths[0] + 5 != 5
