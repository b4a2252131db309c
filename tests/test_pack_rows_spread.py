"""pack_rows_kernel with its row_map fill spread over the rows (csrc/attention.hip): every workgroup repeats the scan of kmax and fills
its own slices of row_map; workgroup 0 writes cu and cls_rows.  The contract of the three arrays is the comment above the kernel,
restated here in numpy and compared in full through om_debug_pack_rows."""
import numpy as np
import pytest
import torch

from openmatch_amd import native as N

DEV = "cuda:0"
FILL = -7


def contract(kmax, L, rows):
    """cu [B + 2], cls_rows [B], row_map [rows] as the comment above pack_rows_kernel states them"""
    B = kmax.size
    start = np.concatenate([[0], np.cumsum(kmax.astype(np.int64))])      # exclusive scan, then the total
    total = int(start[B])
    cu = np.concatenate([np.minimum(start, rows), [total]])              # offsets clamped to the bound; cu[B + 1] the true count
    cls = np.where(start[:B] < rows, start[:B], rows - 1)
    tok = np.repeat(np.arange(B, dtype=np.int64) * L - start[:B], kmax) + np.arange(total, dtype=np.int64)      # b * L + position
    row_map = np.full(rows, -1, np.int64)
    n = min(total, rows)
    row_map[:n] = tok[:n]
    return cu.astype(np.int32), cls.astype(np.int32), row_map.astype(np.int32)


def test_contract_restatement_on_a_hand_case():
    cu, cls, row_map = contract(np.array([2, 1, 3], np.int32), 4, 8)
    assert cu.tolist() == [0, 2, 3, 6, 6] and cls.tolist() == [0, 2, 3] and row_map.tolist() == [0, 1, 4, 8, 9, 10, -1, -1]
    cu, cls, row_map = contract(np.array([2, 1, 3], np.int32), 4, 2)      # a bound that is too small
    assert cu.tolist() == [0, 2, 2, 2, 6] and cls.tolist() == [0, 1, 1] and row_map.tolist() == [0, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 7, 1024, 3000])
def test_pack_rows_matches_the_contract(B):
    """L in {1, 128, 512}; kmax random, all 1, all L; the exact bound, the loose bound roundup256(B L), one row too few and half
    the rows (where that leaves a legal bound of at least 1): cu, cls_rows and row_map equal the numpy result in full, and nothing is
    written at or past `rows`"""
    rng = np.random.default_rng(100 + B)
    lib = N.lib()
    guard = 64
    for L in (1, 128, 512):
        for kname, kmax in (("random", rng.integers(1, L + 1, B)), ("ones", np.ones(B, np.int64)), ("full", np.full(B, L))):
            kmax = kmax.astype(np.int32)
            total = int(kmax.sum())
            kd = torch.from_numpy(kmax).to(DEV)
            for rows in (total, (B * L + 255) // 256 * 256, total - 1, total // 2):
                if rows < 1:
                    continue
                cu = torch.full((B + 2,), FILL, dtype=torch.int32, device=DEV)
                cls = torch.full((B,), FILL, dtype=torch.int32, device=DEV)
                row_map = torch.full((rows + guard,), FILL, dtype=torch.int32, device=DEV)
                with torch.cuda.device(DEV):
                    N.check(lib.om_debug_pack_rows(N.ptr(kd), B, L, rows, N.ptr(cu), N.ptr(cls), N.ptr(row_map), N.stream_ptr(torch.device(DEV))))
                torch.cuda.synchronize()
                e_cu, e_cls, e_map = contract(kmax, L, rows)
                label = (B, L, kname, rows, total)
                assert np.array_equal(cu.cpu().numpy(), e_cu), label
                assert np.array_equal(cls.cpu().numpy(), e_cls), label
                got = row_map.cpu().numpy()
                assert np.array_equal(got[:rows], e_map), label
                assert (got[rows:] == FILL).all(), label
