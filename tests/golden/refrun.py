"""What the seven generators tests/golden/make_ref_*.py share: building a program of oracle/_ref (oracle/ref/Makefile), packing its
in.bin, running it in a scratch directory and reading its out.bin, and the helpers that put block arrays into the records' form.
The builds and runs work in the build container only (the reference does not travel); the helpers are used by the tests as well."""
from __future__ import annotations

import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFDIR = os.path.join(ROOT, "oracle", "ref")
# the make target that builds each program (`kernels` builds ref_kernels and ref_remap together)
TARGET = {"ref_harness": "all", "ref_kernels": "kernels", "ref_remap": "kernels", "ref_ridge": "ridge", "ref_itd": "itd", "ref_therm2": "therm2",
          "ref_shortwave": "shortwave"}
# the tracer indices and switches ref_therm2.F90 reads, in its order; ref_itd.F90 reads the same without nt_sice and nt_FY
IDX = ("nt_Tsfc", "nt_qice", "nt_qsno", "nt_sice", "nt_alvl", "nt_vlvl", "nt_apnd", "nt_hpnd", "nt_fbri", "nt_iage", "nt_FY", "tr_pond_cesm",
       "tr_pond_lvl", "tr_pond_topo", "tr_brine")


def exe(program, cfg):
    return os.path.join(ROOT, "oracle", "_ref", cfg, program)


def build(program, cfg, dims, ncat, layers=(4, 1)):
    """makes oracle/_ref/<cfg>/<program> for dims = (nx, ny, bx, by, mxb), ncat categories and layers = (nilyr, nslyr); returns its path"""
    nx, ny, bx, by, mxb = dims
    subprocess.check_call(["make", "-C", REFDIR, TARGET[program], f"CFG={cfg}", f"NX={nx}", f"NY={ny}", f"BX={bx}", f"BY={by}", f"MXB={mxb}",
                           f"NCAT={ncat}", f"NILYR={layers[0]}", f"NSLYR={layers[1]}"], stdout=subprocess.DEVNULL)
    return exe(program, cfg)


class Writer:
    def __init__(self):
        self.parts = []

    def i4(self, *v):
        self.parts.append(np.asarray(v, dtype=np.int32).tobytes())

    def r8(self, *v):
        self.parts.append(np.asarray(v, dtype=np.float64).tobytes())

    def arr(self, a):
        self.parts.append(np.ascontiguousarray(a).tobytes())

    def raw(self, b):
        self.parts.append(b)

    def payload(self):
        return b"".join(self.parts)


class Reader:
    def __init__(self, buf):
        self.b, self.o = buf, 0

    def take(self, dtype, shape):
        n = int(np.prod(shape)) if shape else 1
        a = np.frombuffer(self.b, dtype=dtype, count=n, offset=self.o).reshape(shape).copy()
        self.o += a.nbytes
        return a

    def done(self):
        assert self.o == len(self.b), (self.o, len(self.b))


def domain_nml(ew, ns):
    return ("&domain_nml\n  nprocs = 1\n  processor_shape = 'slenderX1'\n  distribution_type = 'cartesian'\n"
            f"  distribution_wght = 'latitude'\n  ew_boundary_type = '{ew}'\n  ns_boundary_type = '{ns}'\n"
            "  maskhalo_dyn = .false.\n  maskhalo_remap = .false.\n  maskhalo_bound = .false.\n/\n")


def run(exe, payload, nml=None):
    """the program on in.bin = payload (and cice_in.nml = nml) in a scratch directory: (Reader on its out.bin, text of out.bin.diag or
    None); an AssertionError with the tail of its output if it fails"""
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "in.bin"), "wb") as f:
            f.write(payload)
        if nml is not None:
            with open(os.path.join(td, "cice_in.nml"), "w") as f:
                f.write(nml)
        p = subprocess.run([exe, "in.bin", "out.bin"], cwd=td, capture_output=True, text=True)
        out = os.path.join(td, "out.bin")
        assert p.returncode == 0 and os.path.exists(out), p.stdout[-800:] + p.stderr[-800:]
        with open(out, "rb") as f:
            r = Reader(f.read())
        diag = open(out + ".diag").read() if os.path.exists(out + ".diag") else None
    return r, diag


def padded(a, mxb):
    """a (nblocks, ...) on the reference's max_blocks blocks, zero beyond nblocks"""
    out = np.zeros((mxb,) + a.shape[1:], dtype=a.dtype)
    out[:len(a)] = a
    return out


def on_cells(a, m):
    """values of a block array on the cells of mask m (nb, ny, nx), (block, j, i) order, the category / tracer axes last"""
    if a.ndim == 3:
        return a[m]
    return np.moveaxis(a, (0, -2, -1), (0, 1, 2))[m]


def same(a, b):
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all()) if a.dtype.kind == "f" else np.array_equal(a, b)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else np.ascontiguousarray(a)
