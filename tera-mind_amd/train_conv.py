"""The conv engine of the training path -- forward, data gradient and weight gradient of Conv3d(3x3x3 pad 1 | 1x1x1) on CB8 tensors [N,
ceil(C/8), Z, S, S, 8]: one interface, two implementations -- and the flat parameter layout.  The only module that names the conv entry
points of the C-ABI: ResBlockTrain, AttnBlockTrain, DownZTrain (training.py) and UNetTrain.conv (train_model.py) call an engine.

    f  = eng.filter(wid, weight, dz=None)     a weight [Co, Ci] or [Co, Ci, kz, ky, kx] as the engine takes it (ConvFilter)
    y  = eng.conv(x_cb, f, bias, out=None)    forward
    dx = eng.dgrad(g_cb, f)                   data gradient: the forward kernel on the flipped, transposed filter
    dw, db = eng.wgrad(x_cb, g_cb, f, dw=None, db=None, accumulate=0)      weight / bias gradient into tensors on eng.gdev (fresh ones when
                                              dw is None; with dw given db may be omitted); a tap gets the whole 3x3x3 gradient
    eng.wgrad_into(grads, gacc, kw, kb, x_cb, g_cb, f)                     wgrad homed in a gradient dict by the engine's own policy

HostConvs: host weights and biases, packed and uploaded by every call (tm_op_conv_mfma / _dgrad / _wgrad), every call synchronises;
gradients land in fresh host tensors and the caller adds on the host.  ResidentConvs: device weights and biases (views of a parameter
arena), packed on the device once per role (0 forward, 1 data gradient) on first use after invalidate() (tm_op_conv_pack_dev) and read
by tm_op_conv_mfma_packed / tm_op_conv_dgrad_packed; tm_op_conv_wgrad_dev writes, or with accumulate = 1 adds, into a device tensor;
nothing synchronises, no host memory is touched.  Packs are cached by (wid, role), wid a state-dict key prefix (counted in pack_count)
or (prefix, dz) for a down_z tap.

Geometry (N, Z, S from the CB8 tensor; Co, Ci, ksize from the filter) is derived here.  The k x 3 x 3 kernels take planes of S = 4 ..
128: a 2 x 2 plane (the gene grid of patch size 32) runs in the corner of a zero 4 x 4 plane, whose zeros right of and below the corner
are the conv's own zero padding: the corner of the result is the 'same' conv of the 2 x 2 plane, forward and data gradient alike (a
re-indexing, no arithmetic).  The weight gradient kernels take any S and read the tensors as they are.

Lifetime rules of the asynchronous calls, obeyed in ResidentConvs and nowhere else:
  1. every tensor whose pointer goes into a queued call is bound to a local name until the call has returned: a temporary would be
     released as soon as its pointer is taken, and a later allocation of the same statement could take its memory;
  2. in the data gradient the pack is obtained before the padded gradient is made: a pack built on a miss (and the embedded filter it
     is built from) is never allocated between the padded gradient and the call that reads it.
"""
import collections
import ctypes as C
import math

import torch
import torch.nn.functional as F

from . import _lib


def _hp(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)


def embed_133(w33: torch.Tensor) -> torch.Tensor:
    """w33 [Co, Ci, 3, 3] -> the 3x3x3 filter that is zero but for w33 in its middle z plane, on w33's device"""
    wf = torch.zeros((w33.shape[0], w33.shape[1], 3, 3, 3), dtype=torch.float32, device=w33.device)
    wf[:, :, 1] = w33
    return wf


class ParamLayout:
    """The flat fp32 parameter arena: the tensors of a state dict back to back in its key order.  keys, shape[key], off[key], n."""

    def __init__(self, params: dict):
        self.keys = list(params)
        self.shape = {k: tuple(params[k].shape) for k in self.keys}
        self.off, self.n = {}, 0
        for k in self.keys:
            self.off[k] = self.n
            self.n += math.prod(self.shape[k])

    def flatten(self, d: dict) -> torch.Tensor:
        return torch.cat([d[k].reshape(-1) for k in self.keys])

    def view(self, flat: torch.Tensor, key: str) -> torch.Tensor:
        return flat[self.off[key]:self.off[key] + math.prod(self.shape[key])].reshape(self.shape[key])

    def split(self, flat: torch.Tensor) -> dict:
        return {k: self.view(flat, k) for k in self.keys}


class ConvFilter:
    """A conv weight as an engine takes it.  w: as stored; dz: the z tap that runs as an in-plane conv embedded in a 3x3x3 one (0 for a (1,3,3)
    weight, None for 3x3x3 / 1x1x1 / Linear weights); gshape: of the gradient the kernels write; wf: the kernel's form, kept (host engine)."""
    __slots__ = ("wid", "w", "dz", "co", "ci", "ks", "gshape", "wf")

    def __init__(self, wid, w, dz, keep_form):
        kshape = tuple(w.shape[2:])
        self.wid, self.w = wid, w
        self.co, self.ci = w.shape[:2]
        self.ks = 1 if kshape in ((), (1, 1, 1)) else 3
        self.dz = 0 if dz is None and kshape == (1, 3, 3) else dz
        self.gshape = (self.co, self.ci, 3, 3, 3) if self.ks == 3 else tuple(w.shape)
        if self.ks == 3 and (kshape[1:] != (3, 3) or self.dz is None and kshape[0] != 3):
            raise ValueError(f"conv weight {wid}: kernel {kshape} is neither 1x1x1, 3x3x3 nor a z tap of (kz, 3, 3)")
        self.wf = self.kernel_form() if keep_form else None

    def kernel_form(self):
        return self.w.contiguous() if self.dz is None else embed_133(self.w[:, :, self.dz])


class _Convs:
    """what the engines share: geometry, output allocation, the 2 x 2 plane rule; _conv / _dgrad / _wgrad are the engine's calls"""

    def __init__(self, device):
        self.dev = torch.device(device)
        self.gdev = self.dev if self.resident else torch.device("cpu")  # where wgrad's results live
        self._packs = {}                                          # resident: (wid, role) -> (pack, Z)
        self.pack_count = collections.Counter()                         # resident: (conv key, role) -> packs built so far

    def filter(self, wid, w, dz=None):
        return ConvFilter(wid, w, dz, keep_form=not self.resident)

    def invalidate(self):
        """the weights changed in place (an optimizer step on the arena): every pack is stale"""
        self._packs.clear()

    @staticmethod
    def _geo(t_cb, f):
        N, Z, S = t_cb.shape[0], t_cb.shape[2], t_cb.shape[3]
        return N, Z, S, 4 if f.ks == 3 and S == 2 else S            # and Sc, the plane the kernels run it at (the 2 x 2 plane rule)

    @staticmethod
    def _corner_in(t, S, Sc):
        return t if Sc == S else F.pad(t, (0, 0, 0, Sc - S, 0, Sc - S)).contiguous()

    @staticmethod
    def _corner_out(t, S, Sc):
        return t if Sc == S else t[:, :, :, :S, :S].contiguous()

    def conv(self, x_cb, f, bias, out=None):
        N, Z, S, Sc = self._geo(x_cb, f)
        assert out is None or Sc == S
        xin = self._corner_in(x_cb, S, Sc)
        y = torch.zeros((N, (f.co + 7) // 8, Z, Sc, Sc, 8), dtype=torch.float32, device=self.dev) if out is None else out
        self._conv(xin, f, bias, y, N, Z, Sc)
        return self._corner_out(y, S, Sc)

    def dgrad(self, g_cb, f):
        N, Z, S, Sc = self._geo(g_cb, f)
        dx = torch.zeros((N, (f.ci + 7) // 8, Z, Sc, Sc, 8), dtype=torch.float32, device=self.dev)
        self._dgrad(g_cb, f, dx, N, Z, S, Sc)
        return self._corner_out(dx, S, Sc)

    def wgrad(self, x_cb, g_cb, f, dw=None, db=None, accumulate=0):
        if dw is None:
            dw = torch.empty(f.gshape, dtype=torch.float32, device=self.gdev)
            db = torch.empty((f.co,), dtype=torch.float32, device=self.gdev)
        self._wgrad(x_cb, g_cb, f, dw, db, accumulate, *self._geo(x_cb, f)[:3])
        return dw, db


class HostConvs(_Convs):
    resident = False

    def _conv(self, xin, f, bias, y, N, Z, Sc):
        _call("tm_op_conv_mfma", _lib.ptr(xin), _hp(f.wf), _hp(bias), _lib.ptr(y), N, f.ci, f.co, Z, Sc, f.ks, 0, 0, 0)

    def _dgrad(self, g_cb, f, dx, N, Z, S, Sc):
        gin = self._corner_in(g_cb, S, Sc)
        _call("tm_op_conv_dgrad", _lib.ptr(gin), _hp(f.wf), _lib.ptr(dx), N, f.ci, f.co, Z, Sc, f.ks)

    def _wgrad(self, x_cb, g_cb, f, dw, db, accumulate, N, Z, S):
        assert not accumulate, "the host weight gradient overwrites: the caller adds on the host"
        _call("tm_op_conv_wgrad", _lib.ptr(x_cb), _lib.ptr(g_cb), _hp(dw), _hp(db), N, f.ci, f.co, Z, S, f.ks)

    def wgrad_into(self, grads, gacc, kw, kb, x_cb, g_cb, f):
        dw, db = self.wgrad(x_cb, g_cb, f)
        gacc(kw, dw if f.dz is None else dw[:, :, 1:2].contiguous())
        gacc(kb, db)


class ResidentConvs(_Convs):
    resident = True

    def _pack(self, f, role, Z):
        hit = self._packs.get((f.wid, role))
        if hit is not None:
            assert hit[1] == Z, (f.wid, hit[1], Z)
            return hit[0]
        wf = f.kernel_form()
        pk = torch.empty((_lib.lib().tm_conv_pack_floats(f.co, f.ci, f.ks, Z, role),), dtype=torch.float32, device=self.dev)
        _call("tm_op_conv_pack_dev", _lib.ptr(wf), _lib.ptr(pk), f.co, f.ci, f.ks, Z, role)
        self._packs[(f.wid, role)] = (pk, Z)
        if isinstance(f.wid, str):
            self.pack_count[(f.wid, role)] += 1
        return pk

    def _conv(self, xin, f, bias, y, N, Z, Sc):
        pk = self._pack(f, 0, Z)
        _call("tm_op_conv_mfma_packed", _lib.ptr(xin), _lib.ptr(pk), _lib.ptr(bias), _lib.ptr(y), N, f.ci, f.co, Z, Sc, f.ks)

    def _dgrad(self, g_cb, f, dx, N, Z, S, Sc):
        pk = self._pack(f, 1, Z)                                        # rule 2: before gin
        gin = self._corner_in(g_cb, S, Sc)
        _call("tm_op_conv_dgrad_packed", _lib.ptr(gin), _lib.ptr(pk), _lib.ptr(dx), N, f.ci, f.co, Z, Sc, f.ks)

    def _wgrad(self, x_cb, g_cb, f, dw, db, accumulate, N, Z, S):
        _call("tm_op_conv_wgrad_dev", _lib.ptr(x_cb), _lib.ptr(g_cb), _lib.ptr(dw), _lib.ptr(db), accumulate, N, f.ci, f.co, Z, S, f.ks)

    def wgrad_into(self, grads, gacc, kw, kb, x_cb, g_cb, f):
        """straight into grads[kw] / grads[kb], accumulate = 1 for a weight's second use in one backward; a tap's gradient is sliced on the device"""
        acc = 1 if kw in grads else 0
        if not acc:
            grads[kb] = torch.empty((f.co,), dtype=torch.float32, device=self.dev)
        if f.dz is not None:
            dw = (torch.zeros if acc else torch.empty)(f.gshape, dtype=torch.float32, device=self.dev)
        else:
            if not acc:
                grads[kw] = torch.empty(f.gshape, dtype=torch.float32, device=self.dev)
            dw = grads[kw]
        self.wgrad(x_cb, g_cb, f, dw, grads[kb], acc)
        if f.dz is not None:
            gacc(kw, dw[:, :, 1:2])
