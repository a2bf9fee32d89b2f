// rectify_plan_check.cc — sdvl_stereo_rectify_plan (csrc/rectify_plan.cc) compiled on its own: standard library only, no device, no
// library of the project's.  tests/test_rectify_restatement_cpu.py runs it against the plan's restatement in numpy.
//   rectify_plan_check fx1 fy1 u01 v01 d1[5] fx2 fy2 u02 v02 d2[5] R[9] T[3] width height [fx fy u0 v0]
// (the last four: the override).  Prints "refused CODE" or the plan, one value a line at 17 significant digits: R1[9], R2[9], the
// rectified fx fy u0 v0, the baseline; exit code 0 either way, 2 for a malformed command line.
#include <cstdio>
#include <cstdlib>

#include "../csrc/rectify_plan.cc"

int main(int argc, char **argv) {
  if (argc != 1 + 32 && argc != 1 + 36) {
    std::fprintf(stderr, "rectify_plan_check: 32 or 36 numbers, got %d\n", argc - 1);
    return 2;
  }
  double v[36];
  for (int i = 1; i < argc; i++) {
    char *end = nullptr;
    v[i - 1] = std::strtod(argv[i], &end);
    if (end == argv[i] || *end != 0) {
      std::fprintf(stderr, "rectify_plan_check: not a number: %s\n", argv[i]);
      return 2;
    }
  }
  sdvl_stereo_rig rig;
  const double *p = v;
  const auto camera = [&](sdvl_camera *c, sdvl_distortion *d) {
    *c = sdvl_camera{0, 0, p[0], p[1], p[2], p[3]};
    for (int i = 0; i < 5; i++) d->d[i] = p[4 + i];
    p += 9;
  };
  camera(&rig.left, &rig.left_dist);
  camera(&rig.right, &rig.right_dist);
  for (int i = 0; i < 9; i++) rig.R[i] = *p++;
  for (int i = 0; i < 3; i++) rig.T[i] = *p++;
  const int width = static_cast<int>(p[0]), height = static_cast<int>(p[1]);
  p += 2;
  sdvl_camera over{0, 0, 0, 0, 0, 0};
  const bool has_override = argc == 1 + 36;
  if (has_override) over = sdvl_camera{0, 0, p[0], p[1], p[2], p[3]};
  sdvl_stereo_rectified out;
  const int rc = sdvl_stereo_rectify_plan(&rig, width, height, has_override ? &over : nullptr, &out);
  if (rc != 0) {
    std::printf("refused %d\n%s\n", rc, sdvl_stereo_rectify_plan_message(rc));
    return 0;
  }
  for (int i = 0; i < 9; i++) std::printf("%.17g\n", out.left.R[i]);
  for (int i = 0; i < 9; i++) std::printf("%.17g\n", out.right.R[i]);
  std::printf("%.17g\n%.17g\n%.17g\n%.17g\n%.17g\n", out.left.rect.fx, out.left.rect.fy, out.left.rect.u0, out.left.rect.v0, out.baseline);
  return 0;
}
