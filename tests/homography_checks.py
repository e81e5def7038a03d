"""The comparisons every GPU test of findHomography makes: the library against tests/homography_oracle.py, H and every tap bit
for bit, the mask byte for byte; and the upload of a list of point sets for the batched device form."""
import numpy as np

import homography_oracle as HO
from orb_slam2_ssd_semantic_amd import homography as HG


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_taps(hg, set_index, t, name):
    """the taps of set `set_index` of the handle's last call against the oracle's stage results `t`"""
    assert np.array_equal(bits(hg.tap(set_index, HG.TAP_RANSAC)), bits(t["ransac_H"])), name
    info = hg.tap(set_index, HG.TAP_INFO)
    assert list(info) == [int(t["ransac_ok"]), t["iters"], t["niters"], int(t["refit_ok"])], (name, info, t)
    assert np.array_equal(bits(hg.tap(set_index, HG.TAP_REFIT)), bits(t["refit_H"] if t["refit_ok"] else np.zeros(9))), name


def check_case(hg, s, d, kw, name, oracle=None):
    """one host call against the oracle (`oracle`: find_homography(s, d, taps=True, **kw) when the caller has it already)"""
    H, mask = hg.find(s, d, **kw)
    oH, omask, t = oracle if oracle is not None else HO.find_homography(s, d, taps=True, **kw)
    assert (H is None) == (oH is None), name
    if oH is not None:
        assert np.array_equal(bits(H), bits(oH)), (name, H, oH)
    assert np.array_equal(mask, omask), name
    if len(s) >= 4:
        check_taps(hg, 0, t, name)
    return H, t


def batch(hg, sets, min_pairs, **kw):
    """find_batch over [(src, dst)] on device 0, synchronised: (H, ok, mask, offsets) as numpy"""
    import torch
    off = np.r_[0, np.cumsum([len(s) for s, _ in sets])].astype(np.int32)
    src = np.concatenate([s for s, _ in sets] + [np.zeros((0, 2), np.float32)]).astype(np.float32)
    dst = np.concatenate([d for _, d in sets] + [np.zeros((0, 2), np.float32)]).astype(np.float32)
    dev = torch.device("cuda", 0)
    H, ok, mask = hg.find_batch(torch.from_numpy(off).to(dev), torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev),
                                min_pairs=min_pairs, **kw)
    torch.cuda.synchronize()
    return H.cpu().numpy(), ok.cpu().numpy(), mask.cpu().numpy(), off
