// fdcn_qmc_table.h -- host-only checks of the path-construction table of
// fdcn_mc_qmc_batch (include/fdcn.h), kept free of HIP calls so they run on
// the CPU under the sanitizers (tools/sanitize/qmc_check_driver.cpp), as
// fdcn_session_book.h does.  A table that passes keeps every index the path
// kernel forms inside its [n_steps + 1] rows of W, and never reads a row
// before it is written.
#ifndef FDCN_QMC_TABLE_H
#define FDCN_QMC_TABLE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifndef FDCN_QMC_MAX_STEPS
#define FDCN_QMC_MAX_STEPS 64  // include/fdcn.h
#endif

namespace fdcn_qmc {

// bridge_idx [n_steps][3] = target, left, right.  0, or the reason in err and
// -1.  Row j: target in 1 .. n_steps and not a target before; left < target
// and defined (0 or an earlier target); right > target and defined, or
// right == left (an extension past the known range).
inline int check_bridge_idx(int32_t n_steps, const int32_t* idx, char* err, size_t errlen) {
  if (n_steps < 1 || n_steps > FDCN_QMC_MAX_STEPS) {
    snprintf(err, errlen, "n_steps must be in 1 .. %d", FDCN_QMC_MAX_STEPS);
    return -1;
  }
  if (!idx) {
    snprintf(err, errlen, "bridge_idx is NULL");
    return -1;
  }
  bool defined[FDCN_QMC_MAX_STEPS + 1] = {};
  defined[0] = true;
  for (int32_t j = 0; j < n_steps; ++j) {
    const int32_t t = idx[3 * j], l = idx[3 * j + 1], r = idx[3 * j + 2];
    if (t < 1 || t > n_steps) {
      snprintf(err, errlen, "bridge_idx row %d: target %d is outside 1 .. %d", j, t, n_steps);
      return -1;
    }
    if (defined[t]) {
      snprintf(err, errlen, "bridge_idx row %d: target %d is set twice", j, t);
      return -1;
    }
    if (l < 0 || l >= t) {
      snprintf(err, errlen, "bridge_idx row %d: left %d is not in 0 .. target - 1", j, l);
      return -1;
    }
    if (!defined[l]) {
      snprintf(err, errlen, "bridge_idx row %d: left %d is not defined yet", j, l);
      return -1;
    }
    if (r != l) {
      if (r <= t || r > n_steps) {
        snprintf(err, errlen,
                 "bridge_idx row %d: right %d is neither above target %d (up to %d) nor left", j, r,
                 t, n_steps);
        return -1;
      }
      if (!defined[r]) {
        snprintf(err, errlen, "bridge_idx row %d: right %d is not defined yet", j, r);
        return -1;
      }
    }
    defined[t] = true;
  }
  return 0;
}

// bridge_w [B][n_steps][3] (host memory): every weight finite
inline int check_bridge_w(int32_t B, int32_t n_steps, const double* w, char* err, size_t errlen) {
  const size_t n = (size_t)B * (size_t)n_steps * 3;
  for (size_t k = 0; k < n; ++k)
    if (!isfinite(w[k])) {
      snprintf(err, errlen, "bridge_w of contract %d, row %d is not finite",
               (int)(k / ((size_t)n_steps * 3)), (int)(k / 3 % (size_t)n_steps));
      return -1;
    }
  return 0;
}

}  // namespace fdcn_qmc

#endif  // FDCN_QMC_TABLE_H
