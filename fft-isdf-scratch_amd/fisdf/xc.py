"""The functionals the device evaluates (csrc/func.hip: fisdf_xc_eval, fisdf_nr_rks_block) and
their names.  Spin-unpolarised only: Slater exchange + PW92 correlation ("pw_mod" parameters) for
LDA, PBE for GGA, with the exchange and correlation parts scaled by ``cx`` and ``cc`` and ``hyb``
the fraction of exact exchange a hybrid adds (``vxc + vj - 0.5 * hyb * vk``).  Anything else goes
through a callable ``f(rho_block) -> (e_block, wv_block)`` (ISDF.nr_rks).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

LDA, GGA = 0, 1
FAMILIES = {"LDA": LDA, "GGA": GGA}

_Functional = namedtuple("Functional", "family cx cc hyb")


class Functional(_Functional):
    """(family, cx, cc, hyb): family "LDA", "GGA" or None (nothing local); e = cx e_x + cc e_c."""
    __slots__ = ()

    def __new__(cls, family, cx=1.0, cc=1.0, hyb=0.0):
        if isinstance(family, str):
            family = family.upper()
        if family is not None and family not in FAMILIES:
            raise ValueError(f"Functional: family must be one of {list(FAMILIES)} or None, "
                             f"not {family!r}")
        cx, cc, hyb = float(cx), float(cc), float(hyb)
        if not (np.isfinite(cx) and np.isfinite(cc) and np.isfinite(hyb)):
            raise ValueError("Functional: cx, cc and hyb must be finite")
        return super().__new__(cls, family, cx, cc, hyb)

    @property
    def code(self):
        """FISDF_XC_LDA / FISDF_XC_GGA of include/fisdf.h (None: nothing local)."""
        return None if self.family is None else FAMILIES[self.family]

    @property
    def local(self):
        return self.family is not None and (self.cx != 0.0 or self.cc != 0.0)


FUNCTIONALS = {
    "lda": Functional("LDA", 1.0, 1.0, 0.0),      # Slater + PW92 (pw_mod)
    "pbe": Functional("GGA", 1.0, 1.0, 0.0),
    "pbe0": Functional("GGA", 0.75, 1.0, 0.25),
    "hf": Functional(None, 0.0, 0.0, 1.0),
}
ALIASES = {"pbe,pbe": "pbe"}


def parse_xc(xc):
    """The table entry of a functional's name (case-insensitive; "pbe,pbe" is "pbe"), or a
    Functional as it is.  Anything else raises ValueError naming the known ones."""
    if isinstance(xc, Functional):
        return xc
    if isinstance(xc, str):
        key = xc.strip().lower().replace(" ", "")
        key = ALIASES.get(key, key)
        if key in FUNCTIONALS:
            return FUNCTIONALS[key]
    raise ValueError(f"unknown functional {xc!r}: the device evaluates {sorted(FUNCTIONALS)} "
                     f"(and {sorted(ALIASES)}), spin-unpolarised; build a mix with "
                     "fisdf.xc.Functional(family, cx, cc, hyb) or pass a callable "
                     "f(rho) -> (e, wv) to nr_rks")


def hybrid_coeff(xc):
    """The fraction of exact exchange of a functional (0 for a callable)."""
    return 0.0 if callable(xc) and not isinstance(xc, Functional) else parse_xc(xc).hyb


def nr_rks_arena(nk, ng, nao, nset):
    """(bytes per point, fixed bytes) of the arena of one fused block (fisdf_nr_rks_plan; needs
    the library, not a device)."""
    from . import _lib
    pp, fx = C.c_long(), C.c_long()
    rc = _lib.load().fisdf_nr_rks_plan(int(nk), int(ng), int(nao), int(nset), C.byref(pp),
                                       C.byref(fx))
    _lib.check(rc)
    return pp.value, fx.value
