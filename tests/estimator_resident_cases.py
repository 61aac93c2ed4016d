"""What tests/test_estimator_resident_cpu.py and tests/test_gpu_estimator_resident.py share: the plain-numpy
restatement of "flags from marks" as gmg_refine_forest_marked defines it, and the estimator's small inputs for a forest of
tests/refine_cases.py."""
from types import SimpleNamespace

import numpy as np

import kelly_reference as kr


def active_number(fc):
    """per cell of all levels, in (level, index) order: the number of active cells before it (the exclusive count)"""
    active = np.asarray(fc.cell_first_child, dtype=np.int64).reshape(-1) < 0
    return np.concatenate(([0], np.cumsum(active)))[:-1], active


def flags_from_marks(fc, marks):
    """flag[c] = first_child[c] < 0 ? mark[active number of c] : 0"""
    number, active = active_number(fc)
    marks = np.asarray(marks, dtype=np.uint8).reshape(-1)
    assert len(marks) == int(active.sum()), (len(marks), int(active.sum()))
    flag = np.zeros(len(active), dtype=np.uint8)
    for c in range(len(active)):
        if active[c]:
            flag[c] = marks[number[c]]
    return flag


def marks_of_flags(fc, flag):
    """the marks of the active cells in (level, index) order, read off a flag array (flags on inactive cells are not marks)"""
    active = np.asarray(fc.cell_first_child, dtype=np.int64).reshape(-1) < 0
    return (np.asarray(flag, dtype=np.uint8).reshape(-1)[active] != 0).astype(np.uint8)


def level_tables(dim, h0, ng, nq1):
    """the per-level factors as the driver forms them, the 1-D Gauss rule on [0, 1] and the tensor weights of nq1^dim points"""
    h = h0 / 2.0 ** np.arange(16)
    gx, gw = kr.gauss01(ng)
    _, w1 = kr.gauss01(nq1)
    w = np.ones(1)
    for _ in range(dim):
        w = np.multiply.outer(w1, w).reshape(-1)
    return SimpleNamespace(h_of_level=h, face_measure_of_level=h ** (dim - 1), diameter_of_level=h * np.sqrt(float(dim)), jxw_of_level=h ** dim,
                           gauss_x=gx, gauss_w=gw, weight=w, nq=len(w))
