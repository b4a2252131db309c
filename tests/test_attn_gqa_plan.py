"""The grouped-query attention planner (csrc/attn_plan.h attn_plan_gqa) through its host-only hook om_debug_attention_gqa_plan: no GPU.

omk_attention_gqa launches what this plan names -- the causal kernels of the Llama / Qwen2 (head_dim 64) and Qwen3 (128) stacks and the
bidirectional ones of Gemma3 (256) -- so the family, the body, the grid and the dynamic LDS bytes of every call are checked here, and
every refusal by its text.  Every expected value below is written out from the rules of DESIGN.md 4c ("Grouped-query forward"), none is
computed by a second call into the library."""
import ctypes as C

from openmatch_amd import native as N

F32, BF16, F16 = N.OM_F32, N.OM_BF16, N.OM_F16
NAME = {F32: "float32", BF16: "bfloat16", F16: "float16"}
FAM_NAME = {v: k for k, v in N.GQA_FAMILY.items()}

# dynamic LDS bytes by (head_dim, float32 body?): DESIGN.md section 4
LDS = {(64, False): 33280, (64, True): 67584, (128, False): 66048, (128, True): 136192, (256, False): 65792, (256, True): 136960}
# 128-query blocks (grid.y) of a padded length
BLOCKS = {1: 1, 127: 1, 128: 1, 129: 2, 640: 5, 1024: 8}
# head_dim 256: (half window, family) per padded length -- w = 0, 1, L - 2, L - 1 and one w >= L; the band is 0 < w < L - 1
WINDOWS = {
    1: [(0, "full256"), (1, "full256"), (-1, "full256"), (6, "full256")],                                    # L - 1 = 0, L - 2 = -1
    127: [(0, "full256"), (1, "band256"), (125, "band256"), (126, "full256"), (127, "full256")],
    128: [(0, "full256"), (1, "band256"), (126, "band256"), (127, "full256"), (4096, "full256")],
    129: [(0, "full256"), (1, "band256"), (127, "band256"), (128, "full256"), (129, "full256")],
    640: [(0, "full256"), (1, "band256"), (638, "band256"), (639, "full256"), (1000, "full256")],
    1024: [(0, "full256"), (1, "band256"), (1022, "band256"), (1023, "full256"), (1024, "full256")],
}
# (B, heads, kv_heads, grid.x = heads * B): one grouped shape, one ungrouped
SHAPES = [(5, 9, 3, 45), (7, 4, 4, 28)]


def planned(dtype, B, L, heads, kv, hd, causal, w=0, packed=False, ext=True):
    """(family name, float32 body?, grid x, grid y, LDS bytes); None for an empty batch; the error text for a refusal."""
    out = (C.c_int64 * 5)(*([-7] * 5))
    rc = N.lib().om_debug_attention_gqa_plan(dtype, B, L, heads, kv, hd, int(causal), w, int(packed), int(ext), out)
    if rc < 0:
        assert rc == -1 and list(out) == [0] * 5
        return N.lib().om_last_error()
    assert rc == 0
    if out[0] == 0:
        assert list(out) == [0] * 5
        return None
    return (FAM_NAME[out[0]], bool(out[1]), out[2], out[3], out[4])


def test_plan_table():
    n = 0
    for dtype in (F32, BF16, F16):
        f32 = dtype == F32
        for packed in (False, True):
            for L, blocks in BLOCKS.items():
                for B, heads, kv, gx in SHAPES:
                    for hd, family in ((64, "causal64"), (128, "causal128")):
                        got = planned(dtype, B, L, heads, kv, hd, True, packed=packed)
                        assert got == (family, f32, gx, blocks, LDS[hd, f32]), (NAME[dtype], packed, L, heads, hd, got)
                        n += 1
                    for w, family in WINDOWS[L]:
                        got = planned(dtype, B, L, heads, kv, 256, False, w=w, packed=packed)
                        assert got == (family, f32, gx, blocks, LDS[256, f32]), (NAME[dtype], packed, L, heads, w, got)
                        n += 1
    # 3 formats x 2 forms x 2 shapes x (6 lengths x 2 causal widths + 4 + 5 * 5 windows)
    assert n == 3 * 2 * 2 * (12 + 29) == 492, n
    # the padded form without key extents: no key is padding, the same plan; a negative window is no window
    assert planned(F16, 5, 129, 9, 3, 64, True, ext=False) == ("causal64", False, 45, 2, 33280)
    assert planned(F32, 5, 129, 9, 3, 256, False, w=5, ext=False) == ("band256", True, 45, 2, 136960)
    assert planned(BF16, 5, 129, 9, 3, 128, True, w=-3) == ("causal128", False, 45, 2, 66048)
    # the largest grid.x
    assert planned(F16, 2 ** 31 - 1, 8, 1, 1, 64, True) == ("causal64", False, 2 ** 31 - 1, 1, 33280)


def test_refusals_and_their_order():
    n = 0

    def refused(text, *args, **kw):
        nonlocal n
        got = planned(*args, **kw)
        assert isinstance(got, bytes) and text in got, (text, args, kw, got)
        n += 1

    # rule 1: the dtype, before the empty batch
    refused(b"grouped-query attention: dtype must be OM_F32, OM_BF16 or OM_F16", 7, 1, 128, 4, 2, 64, True)
    refused(b"grouped-query attention: dtype must be OM_F32, OM_BF16 or OM_F16", -1, 0, 128, 4, 2, 256, False)
    # rule 2: an empty batch is nothing to do, whatever else is wrong
    assert planned(F16, 0, 5000, 5, 3, 48, True, w=9, packed=True, ext=False) is None
    assert planned(F32, -4, 0, 0, 0, 64, False) is None
    # rule 3: the kernels that exist
    for hd in (32, 96, 256):
        refused(b"grouped heads: head_dim must be 64 or 128", BF16, 1, 128, 4, 2, hd, True)
    for hd in (64, 128):
        refused(b"causal attention: no window", BF16, 1, 128, 4, 2, hd, True, w=1)
    for hd in (64, 128, 96):
        refused(b"bidirectional grouped-query attention: head_dim must be 256", BF16, 1, 128, 4, 2, hd, False)
    # rule 4: the length, with the family's prefix
    for L in (0, 1025, -1):
        for hd in (64, 128):
            refused(b"causal attention: sequence length must be in [1,1024]", F16, 1, L, 4, 2, hd, True)
        refused(b"attention (head_dim 256): sequence length must be in [1,1024]", F16, 1, L, 4, 2, 256, False)
    # rule 5: the grouping
    for heads, kv in ((4, 3), (4, 0), (0, 1), (4, -1), (2, 4)):
        for hd, causal in ((64, True), (128, True), (256, False)):
            refused(b"grouped heads: n_kv_heads must be at least 1 and divide n_heads", F32, 1, 8, heads, kv, hd, causal)
    # rule 6: packed rows need their offsets (packed is the caller's word, never inferred from the pointer)
    for hd in (64, 128):
        refused(b"causal attention over packed rows: the sequence offsets cu", F16, 1, 8, 4, 2, hd, True, packed=True, ext=False)
    refused(b"attention (head_dim 256) over packed rows: the sequence offsets cu", F16, 1, 8, 4, 2, 256, False, packed=True, ext=False)
    # rule 7: grid.x = heads * B is a 31-bit number
    for B, heads in ((2 ** 31, 1), (2 ** 30, 2), (2 ** 40, 3)):
        for hd in (64, 128):
            refused(b"causal attention: batch too large for one launch", F16, B, 8, heads, 1, hd, True)
        refused(b"attention (head_dim 256): batch too large for one launch", F16, B, 8, heads, 1, 256, False)
    # rule 8: head_dim 256 alone -- L * (heads + 2 kv_heads) * 512 bytes from a sequence's first row is a 31-bit number
    refused(b"attention (head_dim 256): too many heads for one sequence's 32-bit row offsets", BF16, 1, 1024, 2048, 1024, 256, False)
    refused(b"attention (head_dim 256): too many heads for one sequence's 32-bit row offsets", BF16, 1, 512, 4096, 2048, 256, False, packed=True)
    assert planned(BF16, 1, 1024, 2046, 1023, 256, False) == ("full256", False, 2046, 8, 65792)
    assert planned(BF16, 1, 512, 2048, 1024, 256, False, w=9) == ("band256", False, 2048, 4, 65792)
    assert planned(BF16, 1, 1024, 2048, 1024, 128, True) == ("causal128", False, 2048, 8, 66048)
    # several faults at once: the order of the rules
    refused(b"causal attention: sequence length must be in [1,1024]", F16, 1, 1025, 4, 3, 128, True)                  # 4 before 5
    refused(b"attention (head_dim 256): sequence length must be in [1,1024]", F16, 1, 1025, 4, 3, 256, False)
    refused(b"causal attention: sequence length must be in [1,1024]", F16, 1, 0, 4, 2, 128, True, packed=True, ext=False)   # 4 before 6
    refused(b"attention (head_dim 256): sequence length must be in [1,1024]", F16, 1, 0, 4, 2, 256, False, packed=True, ext=False)
    refused(b"grouped heads: head_dim must be 64 or 128", F16, 1, 1025, 4, 3, 96, True)                                # 3 before 4 and 5
    refused(b"grouped heads: n_kv_heads must be at least 1 and divide n_heads", F16, 2 ** 31, 8, 4, 3, 64, True, packed=True, ext=False)   # 5 before 6, 7
    refused(b"causal attention over packed rows: the sequence offsets cu", F16, 2 ** 31, 8, 4, 2, 64, True, packed=True, ext=False)        # 6 before 7
    refused(b"attention (head_dim 256): batch too large for one launch", F16, 2 ** 31, 1024, 2048, 1024, 256, False)   # 7 before 8
    assert n == 2 + 3 + 2 + 3 + 9 + 15 + 3 + 9 + 2 + 8 == 56, n
    assert N.lib().om_debug_attention_gqa_plan(F16, 1, 8, 4, 2, 64, 1, 0, 0, 1, None) != 0 and b"null argument" in N.lib().om_last_error()
