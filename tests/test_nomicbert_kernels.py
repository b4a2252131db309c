"""The device pieces NomicBERT adds to the BERT loops, through their debug hooks against float64 torch: the SwiGLU pass over the
[gate; up] rows of the one FFN1 contraction (csrc/elementwise.hip omk_swiglu_rows), the rotary pass over packed rows (omk_rope with a
row_map, csrc/attention_causal.hip) and the embedding of word + token type without a position table (embed_kernel)."""
import pytest
import torch

from openmatch_amd import native as N
from tests.test_attention_kernels import BF16, DEV, DTYPES, F16, F32, FLOOR, GUARD, NAME, TORCH_DT, U_OUT, bits

pytestmark = pytest.mark.gpu


def _sync():
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,F", [(1, 64), (3, 192), (257, 320), (600, 512)])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_swiglu_rows(dtype, M, F):
    """out[m, j] = silu(in[m, j]) * in[m, F + j] in f32, rounded once.  float32 within 1e-6 relative of float64; 16-bit within one ulp
    of the format (2 * U_OUT relative: one rounding of the f64 result, and f32 arithmetic that may move it across a tie).  Gates of
    +-20 sit in the input: exp(-g) at both tails.  The input -- its columns F .. 2F too -- and the rows after M of the output keep
    their bits."""
    g = torch.Generator().manual_seed(M * 1000 + F)
    x0 = (3.0 * torch.randn(M, 2 * F, generator=g))
    x0[:, 0], x0[:, F // 2], x0[-1, 5], x0[0, F - 1] = 20.0, -20.0, -20.0, 20.0
    x0 = x0.to(TORCH_DT[dtype]).to(DEV)
    x = x0.clone()
    out0 = torch.full((M + GUARD, F), 7.0, dtype=TORCH_DT[dtype], device=DEV)
    out = out0.clone()
    N.check(N.lib().om_debug_swiglu_rows(dtype, N.ptr(x), N.ptr(out), M, F, N.stream_ptr()))
    _sync()
    assert torch.equal(bits(x, dtype), bits(x0, dtype))
    assert torch.equal(bits(out, dtype)[M:], bits(out0, dtype)[M:])
    gate, up = x0[:, :F].double(), x0[:, F:].double()
    ref = gate / (1.0 + torch.exp(-gate)) * up
    got = out[:M].double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    bound = (1e-6 if dtype == F32 else 2 * U_OUT[dtype]) * ref.abs() + FLOOR[dtype]
    print(f"\n[swiglu {NAME[dtype]} {M}x{F}] max err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err / bound).max().item()
    # controls: the halves swapped, and gelu in place of silu, are outside the bound
    assert bool(((up / (1.0 + torch.exp(-up)) * gate - ref).abs() > bound).any())
    assert bool(((torch.nn.functional.gelu(gate) * up - ref).abs() > bound).any())


def test_swiglu_rows_refusals():
    lib = N.lib()
    x = torch.zeros(4, 256, dtype=torch.float16, device=DEV)
    out = torch.zeros(4, 128, dtype=torch.float16, device=DEV)
    for F in (96, 0, 32):
        assert lib.om_debug_swiglu_rows(F16, N.ptr(x), N.ptr(out), 4, F, N.stream_ptr()) != 0
        assert b"multiple of 64" in lib.om_last_error()
    assert lib.om_debug_swiglu_rows(F16, None, N.ptr(out), 4, 128, N.stream_ptr()) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_swiglu_rows(F16, N.ptr(x), None, 4, 128, N.stream_ptr()) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_swiglu_rows(9, N.ptr(x), N.ptr(out), 4, 128, N.stream_ptr()) != 0 and b"dtype" in lib.om_last_error()
    assert lib.om_debug_swiglu_rows(F16, N.ptr(x), N.ptr(out), 0, 128, N.stream_ptr()) == 0          # no rows: nothing to do
    N.check(lib.om_debug_swiglu_rows(F16, N.ptr(x), N.ptr(out), 4, 128, N.stream_ptr()))
    _sync()
    assert torch.equal(out, torch.zeros_like(out))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_rope_over_mapped_rows(dtype):
    """40 rows, L = 16, H = 128 (two heads): the map permutes the rows and marks three of them -1.  A mapped row t carries the bits the
    unmapped pass leaves on the same values at row row_map[t] (position row_map[t] % L); the -1 rows, the V columns and the rows after
    the last keep their bits."""
    M, L, H = 40, 16, 128
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(M + GUARD, 3 * H, generator=g).to(TORCH_DT[dtype]).to(DEV)
    row_map = torch.randperm(M, generator=g).to(torch.int32)
    skipped = [4, 17, 39]
    row_map[skipped] = -1
    kept = [t for t in range(M) if t not in skipped]
    assert len({int(row_map[t]) % L for t in kept}) == L and any(int(row_map[t]) != t for t in kept)
    # the unmapped pass over the same values, laid out token by token
    plain = x0.clone()
    N.check(N.lib().om_debug_rope(dtype, N.ptr(plain), M, L, H, 1000.0, N.stream_ptr()))
    xp = x0.clone()
    for t in kept:
        xp[t] = x0[int(row_map[t])]
    before = xp.clone()
    rm = row_map.to(DEV)
    N.check(N.lib().om_debug_rope_rows(dtype, N.ptr(xp), M, L, H, 1000.0, N.ptr(rm), N.stream_ptr()))
    _sync()
    for t in kept:
        assert torch.equal(bits(xp, dtype)[t], bits(plain, dtype)[int(row_map[t])]), t
    assert not torch.equal(bits(xp, dtype)[kept], bits(before, dtype)[kept])
    for t in skipped:
        assert torch.equal(bits(xp, dtype)[t], bits(before, dtype)[t]), t
    assert torch.equal(bits(xp, dtype)[M:], bits(before, dtype)[M:])
    assert torch.equal(bits(xp, dtype)[:, 2 * H:], bits(before, dtype)[:, 2 * H:])
    lib = N.lib()
    assert lib.om_debug_rope_rows(dtype, N.ptr(xp), M, L, H, 1000.0, None, N.stream_ptr()) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_rope_rows(dtype, N.ptr(xp), M, 1025, H, 1000.0, N.ptr(rm), N.stream_ptr()) != 0
    assert lib.om_debug_rope_rows(dtype, N.ptr(xp), M, L, H, 0.0, N.ptr(rm), N.stream_ptr()) != 0


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_embedding_of_word_and_type_without_positions(dtype):
    """LayerNorm(word[id] + type[tt]) for 7 rows of H = 192, token types 0 and 1, against F.layer_norm in float64: float32 within 1e-5,
    16-bit within one output rounding more.  A position table would change the rows; type ids all zero change the rows of type 1."""
    M, H, vocab = 7, 192, 50
    g = torch.Generator().manual_seed(11)
    word = torch.randn(vocab, H, generator=g).to(DEV)
    typ = torch.randn(2, H, generator=g).to(DEV)
    gam = (1.0 + 0.3 * torch.randn(H, generator=g)).to(DEV)
    bet = (0.1 * torch.randn(H, generator=g)).to(DEV)
    ids = torch.tensor([3, 49, 0, 7, 7, 21, 48], dtype=torch.int64, device=DEV)
    tt = torch.tensor([0, 1, 1, 0, 1, 0, 1], dtype=torch.int64, device=DEV)
    eps = 1e-12

    def run(type_ids, pos=None):
        out = torch.full((M + GUARD, H), 5.0, dtype=TORCH_DT[dtype], device=DEV)
        N.check(N.lib().om_debug_embed(dtype, N.ptr(ids), N.ptr(type_ids) if type_ids is not None else None, N.ptr(word),
                                       N.ptr(pos) if pos is not None else None, N.ptr(typ), N.ptr(gam), N.ptr(bet), N.ptr(out), M, M, H, vocab, 2,
                                       eps, N.stream_ptr()))
        _sync()
        assert bool((out[M:] == 5.0).all())
        return out[:M].double()
    ref = torch.nn.functional.layer_norm(word[ids].double() + typ[tt].double(), (H,), gam.double(), bet.double(), eps)
    got = run(tt)
    err = (got - ref).abs().max().item()
    print(f"\n[embed word + type {NAME[dtype]}] max abs err {err:.2e}")
    tol = 1e-5 * max(1.0, ref.abs().max().item())
    assert bool(((got - ref).abs() <= tol + (0.0 if dtype == F32 else U_OUT[dtype]) * ref.abs()).all()), err
    ref0 = torch.nn.functional.layer_norm(word[ids].double(), (H,), gam.double(), bet.double(), eps)
    assert (ref - ref0).abs().max().item() > 0.1                               # the type rows matter
    zero = run(None)                                                            # no ids: type 0 everywhere
    assert torch.equal(zero[tt.cpu() == 0], got[tt.cpu() == 0]) and (zero[tt.cpu() == 1] - got[tt.cpu() == 1]).abs().max().item() > 1e-2
    pos = torch.randn(M, H, generator=g).to(DEV)
    assert (run(tt, pos) - got).abs().max().item() > 1e-2                      # BERT's case still adds its position rows
