"""Geometry and recorded draws of tests/golden/train_data_ref.npz (minted by tools/make_train_data_golden.py from the
reference's own MBADataset._getimg / _trans), shared with tests/test_gpu_train_data.py.  The source tile is not stored: it is
synth.image_tile(REF_TAG, REF_SHAPE, REF_SEED)."""
REF_TAG, REF_SEED = "train_data_ref/img", 11
REF_ZT, REF_H, REF_W, REF_SDIM = 20, 48, 48, 32
REF_SHAPE = (2 * REF_ZT, REF_H, REF_W)
SPAD = {1: 0, 4: 1, 8: 1, 16: 3}
STAINS = ("all", "DAPI", "PolyT")
SNUMS = (1, 4, 8, 16)
TRANS_STAIN, TRANS_SNUM = "all", 4            # the rot x flip cases recorded through the reference's _trans


def ref_draws(snum):
    """(top, left, snm): both corners of the crop range, both ends of the snm range, one draw inside."""
    e, smax = REF_H - REF_SDIM, REF_ZT + 2 * SPAD[snum] - snum
    return [(0, 0, 0), (e, e, smax), (5, 11, smax // 2)]
