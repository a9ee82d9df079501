"""Plain-Python / numpy restatement of gr::trigger::SchmittTrigger<T, Method, 32>::processOne (algorithm/.../SchmittTrigger.hpp:103-222), the detector of
gr::blocks::basic::SchmittTrigger (blocks/basic/.../Trigger.hpp:45), for NO_INTERPOLATION, BASIC_LINEAR_INTERPOLATION and LINEAR_INTERPOLATION and
T in {int16, int32, float32, float64}.

The state machine runs on Python scalars (a float32 widens to a Python float exactly, so every comparison is the value type's); the fits run step by step in
comp_t (:295: T for the floating types, float32 for the integer ones) on numpy scalars, one rounding per operation, in the reference's order.  What the
reference leaves undefined -- a crossing that is not finite or does not fit the integer it is converted to -- is reported with DEGENERATE, edge_idx 0,
edge_offset 0, and the state flips (include/gr4hip.h "Schmitt trigger")."""
import math

import numpy as np

NO_INTERPOLATION, BASIC_LINEAR_INTERPOLATION, LINEAR_INTERPOLATION, POLYNOMIAL_INTERPOLATION = range(4)
RISING, FALLING, DEGENERATE = 1, 2, 4
N_HISTORY = 32  # Trigger.hpp:45

_F32 = np.float32

# A LINEAR fit of slope zero, for offset 0 and threshold 1 (band -1 ... 1) on a fresh detector.  -2 -> 0.5 at [1] enters the zone; 0.75 and -0.75 stay inside;
# 1.0 at [4] is RISING over (1, -0.75, 0.75, 0.5) newest first, whose sum xy = 3 - 1.5 + 0.75 = 2.25 = n mean_x mean_y = 4 * 1.5 * 0.375 exactly: slope 0,
# crossing -inf.  1 -> -0.5 at [5] enters from above, -2 at [6] is an ordinary FALLING.
ZERO_SLOPE = np.array([-2.0, 0.5, 0.75, -0.75, 1.0, -0.5, -2.0], np.float32)
ZERO_SLOPE.setflags(write=False)


def _round(x: float) -> float:
    """std::round: half away from zero (x is exact as a Python float)"""
    a = abs(x)
    f = math.floor(a)
    if a - f >= 0.5:
        f += 1
    return math.copysign(f, x)


class SchmittTrigger:
    def __init__(self, offset, threshold, method, dtype):
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"dtype {dtype}")
        if method not in (NO_INTERPOLATION, BASIC_LINEAR_INTERPOLATION, LINEAR_INTERPOLATION):
            raise ValueError(f"method {method}")
        self.method = method
        self.integer = self.dtype.kind == "i"
        self.comp = np.float64 if self.dtype == np.dtype(np.float64) else np.float32
        self.set_params(offset, threshold)

    def set_params(self, offset, threshold):
        T = self.dtype.type
        if not (math.isfinite(offset) and math.isfinite(threshold) and threshold >= 0):
            raise ValueError("offset / threshold")
        if self.integer:
            info = np.iinfo(self.dtype)
            if offset != int(offset) or threshold != int(threshold):
                raise ValueError("fractional offset / threshold for an integer type")
            o, t = int(offset), int(threshold)
            if not (info.min <= o - t and o + t <= info.max and info.min <= o <= info.max and t <= info.max):
                raise ValueError("offset +- threshold leaves the type's range")
            self.offset, self.upper, self.lower = o, o + t, o - t
        else:
            o, t = T(offset), T(threshold)  # (:67) in the value type
            self.offset, self.upper, self.lower = o.item(), T(o + t).item(), T(o - t).item()
        self.reset()

    def reset(self):  # (:90-101)
        self.last = False
        self.acc = 0
        self.hist = [0] * N_HISTORY if self.integer else [0.0] * N_HISTORY  # oldest first

    # computeEdgePosition (:133-142)
    def _fit_basic(self, y_prev, y_curr):
        with np.errstate(all="ignore"):
            y1, y2 = _F32(y_prev), _F32(y_curr)
            if y1 == y2:
                return 0, _F32(0), 0
            o = (_F32(self.offset) - y1) / (y2 - y1)
            cp = _F32(-1.0) + o
            if not np.isfinite(cp):
                return 0, _F32(0), DEGENERATE
            r = _round(float(cp))
            if not -2 ** 31 <= r < 2 ** 31:
                return 0, _F32(0), DEGENERATE
            return int(r), cp - _F32(int(r)), 0

    # findCrossingIndexLinearRegression (:294-324) and :198-205; w: the n newest samples, newest first
    def _fit_linear(self, w, n):
        C = self.comp
        with np.errstate(all="ignore"):
            nv = C(n)
            sum_x2 = (nv * (nv - C(1)) * (C(2) * nv - C(1))) / C(6)
            mean_x = C(0.5) * (nv - C(1))
            sum_y, sum_xy = C(0), C(0)
            for i in range(n):
                xi = C((n - 1) - i)
                yi = C(w[i])
                sum_y = sum_y + yi
                sum_xy = sum_xy + xi * yi
            mean_y = sum_y / nv
            numerator = sum_xy - nv * mean_x * mean_y
            denominator = sum_x2 - nv * mean_x * mean_x
            slope = numerator / denominator
            intercept = mean_y - slope * mean_x
            crossing = (C(self.offset) - intercept) / slope
            if not np.isfinite(crossing):
                return 0, _F32(0), DEGENERATE
            if self.integer:  # value_t(crossing) truncates; relativeIndex is value_t: the offset is 0
                info = np.iinfo(self.dtype)
                tr = math.trunc(float(crossing))
                rel = tr - (n - 1)
                if not (info.min <= tr <= info.max and info.min <= rel):
                    return 0, _F32(0), DEGENERATE
                return rel, _F32(0), 0
            rel = crossing - C(n - 1)
            r = _round(float(rel))
            if not -2 ** 31 <= r < 2 ** 31:
                return 0, _F32(0), DEGENERATE
            return int(r), _F32(rel) - _F32(int(r)), 0

    def process(self, x):
        """every sample of x through processOne; returns the edges as a dict of arrays (count, sample, kind, edge_idx, edge_offset, n_fit, flags)"""
        x = np.asarray(x)
        assert x.dtype == self.dtype and x.ndim == 1
        xs = x.tolist()
        up, lo = self.upper, self.lower
        last = self.last
        edges = []
        if self.method == NO_INTERPOLATION:  # (:107-121)
            for i, v in enumerate(xs):
                if not last:
                    if v >= up:
                        last = True
                        edges.append((i, RISING, 0, _F32(0), 0, 0))
                elif v <= lo:
                    last = False
                    edges.append((i, FALLING, 0, _F32(0), 0, 0))
        elif self.method == BASIC_LINEAR_INTERPOLATION:  # (:124-163)
            prev = self.hist[-1]
            for i, v in enumerate(xs):
                if not last:
                    if v >= up:
                        last = True
                        idx, off, fl = self._fit_basic(prev, v)
                        edges.append((i, RISING, idx, off, 2, fl))
                elif v <= lo:
                    last = False
                    idx, off, fl = self._fit_basic(prev, v)
                    edges.append((i, FALLING, idx, off, 2, fl))
                prev = v
        else:  # (:166-222)
            full = self.hist + xs
            acc = self.acc
            prev = self.hist[-1]
            for i, v in enumerate(xs):
                was = acc > 0
                if not was:
                    if not last:
                        if prev <= lo and v > lo:
                            acc = 1
                    elif prev >= up and v < up:
                        acc = 1
                else:
                    acc += 1
                if acc > 0:
                    if (v <= lo) if last else (v >= up):
                        n = min(max(acc, 2), N_HISTORY)
                        w = full[i + N_HISTORY - n + 1:i + N_HISTORY + 1][::-1]
                        idx, off, fl = self._fit_linear(w, n)
                        edges.append((i, FALLING if last else RISING, idx, off, n, fl))
                        last = not last
                        acc = 0
                    elif (v > up) if last else (v < lo):
                        acc = 0
                prev = v
            self.acc = acc
        self.last = last
        self.hist = (self.hist + xs)[-N_HISTORY:]
        return {
            "count": len(edges),
            "sample": np.array([e[0] for e in edges], np.int64),
            "kind": np.array([e[1] for e in edges], np.int32),
            "edge_idx": np.array([e[2] for e in edges], np.int32),
            "edge_offset": np.array([e[3] for e in edges], np.float32),
            "n_fit": np.array([e[4] for e in edges], np.int32),
            "flags": np.array([e[5] for e in edges], np.int32),
        }


def positions(e):
    """sample + lastEdgeIdx + lastEdgeOffset, as qa_SchmittTrigger.cpp:43 forms it"""
    return e["sample"].astype(np.float64) + e["edge_idx"] + e["edge_offset"].astype(np.float64)
