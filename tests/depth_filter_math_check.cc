// depth_filter_math_check.cc — csrc/sdvl_depth_filter.h on its own, built with the host compiler (test_depth_filter_math_cpu.py): the
// loop body the device kernels and the host mapper share, one candidate per line of stdin, its sdvl_depth_out per line of stdout.
// A line holds, as numbers strtod reads (the test writes hex floats, so nothing is rounded on the way):
//   cur_pose[7] ref_pose[7] bearing[3] found px[2]
//   rho sigma2 a b z_range cos_alpha last_distance depth_mean position[3] fixed n_failed
//   width height fx fy u0 v0   px_error_angle min_depth scale_min_dist max_failed
//   measured z_c noise_abs noise_quad
// and the answer: outcome n_failed, then rho sigma2 a b cos_alpha last_distance position[3] as hex floats.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sdvl_depth_filter.h"

static const int kFields = 7 + 7 + 3 + 1 + 2 + 13 + 6 + 4 + 4;

int main() {
  std::vector<char> line(1 << 16);
  int n_items = 0;
  while (fgets(line.data(), static_cast<int>(line.size()), stdin)) {
    double v[kFields];
    char *p = line.data();
    int got = 0;
    for (; got < kFields; got++) {
      char *end = nullptr;
      v[got] = strtod(p, &end);
      if (end == p) break;
      p = end;
    }
    if (got == 0) continue;  // an empty line
    if (got != kFields) {
      fprintf(stderr, "item %d: %d of %d fields\n", n_items, got, kFields);
      return 1;
    }
    const double *cur = v, *ref = v + 7, *bearing = v + 14, *px = v + 18, *s = v + 20, *c = v + 33, *f = v + 39, *m = v + 43;
    const bool found = v[17] != 0.0;
    sdvl_depth_state st = {};
    st.rho = s[0]; st.sigma2 = s[1]; st.a = s[2]; st.b = s[3]; st.z_range = s[4];
    st.cos_alpha = s[5]; st.last_distance = s[6]; st.depth_mean = s[7];
    st.position[0] = s[8]; st.position[1] = s[9]; st.position[2] = s[10];
    st.fixed = static_cast<int32_t>(s[11]);
    st.n_failed = static_cast<int32_t>(s[12]);
    st.track_row = -1;
    const sdvl::Cam cam = {c[0], c[1], c[2], c[3], c[4], c[5]};
    sdvl_depth_params fp = {};
    fp.px_error_angle = f[0]; fp.min_depth = f[1]; fp.scale_min_dist = f[2];
    fp.max_failed = static_cast<int32_t>(f[3]);
    const sdvl_depth_out o = sdvl::depth_filter_item(cur, ref, bearing, found, px, st, cam, fp, m[0] != 0.0, m[1], m[2], m[3]);
    printf("%d %d %a %a %a %a %a %a %a %a %a\n", o.outcome, o.n_failed, o.rho, o.sigma2, o.a, o.b, o.cos_alpha, o.last_distance, o.position[0],
           o.position[1], o.position[2]);
    n_items++;
  }
  return 0;
}
