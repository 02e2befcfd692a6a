"""The rna_slc 16 training fixture, shared by tools/make_train_slc16_golden.py (which mints it from the reference) and
tests/test_gpu_train_slc16.py.

tests/golden/train_grad_slc16_ref.npz: GRAD_CFG of tests/train_cases.py with rna_slc = 16 (every conv at Z = 8; attention at C = 64
with 512-token windows, at C = 128 with 128-token windows; down_z at kz = 9: 16 gene planes in, 8 out), one case in the format of
train_grad_ref.npz."""
SLC16_CFG = dict(net_ch=16, rna_num=37, rna_slc=16)
SLC16_CASES = {"mse_seed3": (3, "mse", (1, 0))}         # (seed, loss type, crop index (ix, iy))
