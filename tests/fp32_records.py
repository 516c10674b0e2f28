"""numpy restatement of the FP32 records of the FP32 fine-level sweeps (vasp_amd/csrc/fsi_block.hip: k_pack_f3, k_pack_sb_f32)
and the ctypes signatures of the shim entry points that run them and the sweep kernels of the all-FP64-storage mode.  Tested on
the CPU in tests/test_fp32_record_layouts.py; the GPU tests (tests/test_gpu_fp32_records.py) check the library against it."""
from __future__ import annotations

import ctypes as C

import numpy as np

import kernel_shim as ks

# argument codes as in kernel_shim._SIGS: p pointer, i int32, l int64, f float, d double
SIGS = {
    "shim_pack_f3": "lppp", "shim_pack_sb_f32": "lppp",
    "shim_sweep_tiled_r3": "ilippppppffpppp", "shim_sweep_tiled_a1": "ilipppppppffpppp",
    "shim_sweep_sb_r": "lpppffpppp",
    "shim_sweep_schur_tiled_f64": "ilippppppddpppp",
}
_CT = {"p": C.c_void_p, "i": C.c_int32, "l": C.c_int64, "f": C.c_float, "d": C.c_double}


def load():
    """the shim with the signatures of the FP32-record entry points set (ks.call then runs them)"""
    lib = ks.load()
    for name, sig in SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = [_CT[c] for c in sig]
        fn.restype = C.c_int
    return lib


def float_bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32)).view(np.uint32)


def pack_f3(v, loc):
    """k_pack_f3: four words per pair, (bits of v0, v1, v2, local index)"""
    v = float_bits(v).reshape(-1, 3)
    rec = np.empty((len(v), 4), dtype=np.uint32)
    rec[:, :3] = v
    rec[:, 3] = np.asarray(loc, dtype=np.uint32)
    return rec.reshape(-1)


def pack_sb_f32(v, col):
    """k_pack_sb_f32: ten words per 3x3 block, (bits of a0 .. a8, column)"""
    v = float_bits(v).reshape(-1, 9)
    rec = np.empty((len(v), 10), dtype=np.uint32)
    rec[:, :9] = v
    rec[:, 9] = np.asarray(col, dtype=np.int64).astype(np.uint32)
    return rec.reshape(-1)


def unpack_f3(rec):
    rec = np.asarray(rec, dtype=np.uint32).reshape(-1, 4)
    return np.ascontiguousarray(rec[:, :3]).view(np.float32), rec[:, 3].astype(np.int64)


def unpack_sb_f32(rec):
    rec = np.asarray(rec, dtype=np.uint32).reshape(-1, 10)
    return np.ascontiguousarray(rec[:, :9]).view(np.float32), rec[:, 9].astype(np.int32).astype(np.int64)
