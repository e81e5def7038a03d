"""The batched Fuse (csrc/orbfe_fuse.hip) where an entry's pair is not found by luck -- empty pairs between full ones, boundaries
inside a search workgroup's four entries --, where a slot is matched from both sides of the replay's 1024-thread stride, and
vpFuseCandidates where the scan of its block counts carries from one chunk of 1024 blocks into the next.  Bit for bit against
tests/fuse_oracle.py; tests/test_fuse_oracle.py shows on the CPU that every case reaches its edge."""
import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as FO
from test_gpu_fuse import GUARD, SENT, _check_cands, _dev, _pair, _run, _same, _want, lm, mt, two  # noqa: F401  (lm, mt, two: fixtures)

pytestmark = pytest.mark.gpu

F = np.float32


# ------------------------------------------------------------------------------------------------ the pair of an entry
@pytest.mark.parametrize("mode", [FO.PLAIN, FO.SIM3], ids=["plain", "sim3"])
def test_pair_lookup_and_a_collision_across_the_replay_stride(lm, two, mode):
    """lists of 0, 1, 0, 0, 3, 1025, 0, 5, 0 entries on alternating keyframes: every entry is searched on its own pair's keyframe
    and pose; an empty pair fuses nothing; position 1024 of the long list meets the slot position 224 matched; the search alone
    gives the same matches"""
    import torch
    from orb_slam2_ssd_semantic_amd import mapping
    cases, blk, world = two
    L = FC.pair_lookup(mode)
    assert all(np.array_equal(L["cases"][b][0]["desc"], cases[b][0]["desc"]) for b in (0, 1))
    pairs = [_pair(row, cases[row][0], world.list_of(row, sel), mode, L["S"][row]) for row, sel in zip(L["rows"], L["sels"])]
    got, (want, res) = _run(lm, blk, world, pairs, 3.0, mode), _want(blk, world, pairs, 3.0, mode)
    _same(got, want, mode)
    assert got["off"].tolist() == [0, 0, 1, 1, 1, 4, 1029, 1029, 1034, 1034]
    first = got["first"].reshape(len(pairs), blk.cap)
    for p, r in enumerate(res):
        if len(pairs[p][3]) == 0:
            assert got["nfused"][p] == 0 and (first[p] == -1).all(), p
    assert sum(int(v > 0) for v in got["nfused"]) >= 3
    s = FC.PAIR_LOOKUP_STRIDE
    e0 = int(got["off"][5])
    m = got["match"][e0 + s]
    assert m >= 0 and 0 <= first[5, m] < s
    ne = len(got["match"])
    m2, d2 = torch.full((ne + GUARD,), SENT, dtype=torch.int32, device="cuda"), torch.full((ne + GUARD,), SENT, dtype=torch.int32, device="cuda")
    keep = [_dev(got["off"].view(np.int32)), _dev(np.concatenate([p[3] for p in pairs])), _dev(np.concatenate([p[4] for p in pairs])),
            _dev(np.array([p[1].reshape(12) for p in pairs], F)), _dev(np.array([p[2] for p in pairs], F)),
            _dev(np.array([p[0] for p in pairs], np.int32))]
    k0 = blk.kfs[0]
    lm.FuseSearch_batch_device(blk.frames, blk.B, mapping.fuse_lists_struct(keep[5], keep[3], keep[4], keep[0], keep[1], ne, len(pairs), keep[2]),
                               blk.cam, world.struct, 3.0, k0["scale_factors"], k0["inv_sigma2"], k0["log_scale"], m2.data_ptr(), d2.data_ptr(), mode)
    torch.cuda.synchronize()
    m2, d2 = m2.cpu().numpy(), d2.cpu().numpy()
    assert (m2[ne:] == SENT).all() and (d2[ne:] == SENT).all(), "written past its end"
    assert np.array_equal(m2[:ne], got["match"]) and np.array_equal(d2[:ne], got["dist"])


# ------------------------------------------------------------------------------------------------ vpFuseCandidates
def _cands_guarded(lm, c, cand_cap):
    import torch
    d = [_dev(c["slot"]), _dev(c["n"]), _dev(c["targets"]), _dev(c["bad"])]
    cand = torch.full((cand_cap + GUARD,), SENT, dtype=torch.int32, device="cuda")
    skip = torch.full((cand_cap + GUARD,), 77, dtype=torch.uint8, device="cuda")
    nc = torch.full((2 + GUARD,), SENT, dtype=torch.int32, device="cuda")
    nkf, cap = c["slot"].shape
    lm.FuseCandidates_device(d[0].data_ptr(), d[1].data_ptr(), nkf, cap, d[2].data_ptr(), len(c["targets"]), c["cur"], d[3].data_ptr(), len(c["bad"]),
                             cand.data_ptr(), skip.data_ptr(), cand_cap, nc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cand, skip, nc = cand.cpu().numpy(), skip.cpu().numpy(), nc.cpu().numpy()
    assert (cand[cand_cap:] == SENT).all() and (skip[cand_cap:] == 77).all() and (nc[2:] == SENT).all(), "written past its end"
    return cand[:cand_cap], skip[:cand_cap], nc[:2]


@pytest.mark.parametrize("ntargets, cap", [(64, 4096), (64, 4100), (65, 4096)])
def test_candidates_scan_carries_into_the_next_chunk(lm, ntargets, cap):
    """1024, 1025 and 1040 blocks: the offsets of the blocks from 1024 on are the sum of the first chunk plus their own; and a short
    output keeps the whole count and is not overrun"""
    c = FC.candidates_case(ntargets, cap)
    wc = _check_cands(lm, c["slot"], c["n"], c["targets"], c["bad"], c["cur"])
    ws = FO.candidates(c["slot"], c["n"], list(c["targets"]), c["bad"], c["cur"])[1]
    total = len(wc)
    cand, skip, nc = _cands_guarded(lm, c, total + 100)
    assert nc.tolist() == [total, total] and np.array_equal(cand[:total], wc) and np.array_equal(skip[:total], ws)
    assert (cand[total:] == SENT).all() and (skip[total:] == 77).all()
    short = total - 1000
    cand, skip, nc = _cands_guarded(lm, c, short)
    assert nc.tolist() == [short, total]
    assert np.array_equal(cand, wc[:short]) and np.array_equal(skip, ws[:short])
