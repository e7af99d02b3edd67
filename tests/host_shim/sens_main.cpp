// Stand-alone program (its own main; never loaded into Python) for the sanitizer run of the inertial-sensor code: reads a model, a sensor
// list and inputs written by tests/test_sensors_host.py, runs the host build's forward and reverse pass (sens_shim.cpp) on them and prints
// a checksum.  Built by the test with -fsanitize=address,undefined.  Test harness only.
//
// Input file (text): n_bodies n_dofs B S, gravity(3) dt, then per body: parent joint_type dof_offset pitch, T_pj(12), T_cj(12), axis(3), mass,
// com(3), inertia(6); then per DOF: damping spring rest; then per sensor: body T(12); then state [2n][B], accel [n][B], field [3][B] and the
// cotangents [9 S][B].
#include <cstdio>
#include <cstdlib>

#include "sens_shim.cpp"

static bool rd(FILE* f, double* p, size_t k) {
  for (size_t i = 0; i < k; i++)
    if (fscanf(f, "%lf", p + i) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <input file>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  int nb = 0, n = 0, B = 0, S = 0;
  if (fscanf(f, "%d %d %d %d", &nb, &n, &B, &S) != 4 || nb < 1 || n < 1 || B < 1 || S < 1) return 2;
  nbl_model_desc d;
  std::memset(&d, 0, sizeof(d));
  d.n_bodies = nb; d.n_dofs = n;
  if (!rd(f, d.gravity, 3) || !rd(f, &d.dt, 1)) return 2;
  std::vector<int32_t> parent(nb), jt(nb), off(nb), sbody(S);
  std::vector<double> pitch(nb), Tpj(12 * nb), Tcj(12 * nb), axis(3 * nb), mass(nb), com(3 * nb), inertia(6 * nb), damping(n), spring(n), rest(n),
      sT(12 * S);
  for (int i = 0; i < nb; i++) {
    if (fscanf(f, "%d %d %d", &parent[i], &jt[i], &off[i]) != 3) return 2;
    if (!rd(f, &pitch[i], 1) || !rd(f, &Tpj[12 * i], 12) || !rd(f, &Tcj[12 * i], 12) || !rd(f, &axis[3 * i], 3) || !rd(f, &mass[i], 1) ||
        !rd(f, &com[3 * i], 3) || !rd(f, &inertia[6 * i], 6))
      return 2;
  }
  for (int j = 0; j < n; j++)
    if (!rd(f, &damping[j], 1) || !rd(f, &spring[j], 1) || !rd(f, &rest[j], 1)) return 2;
  for (int k = 0; k < S; k++)
    if (fscanf(f, "%d", &sbody[k]) != 1 || sbody[k] < -1 || sbody[k] >= nb || !rd(f, &sT[12 * k], 12)) return 2;
  d.parent = parent.data(); d.joint_type = jt.data(); d.dof_offset = off.data(); d.pitch = pitch.data(); d.T_pj = Tpj.data(); d.T_cj = Tcj.data();
  d.axis = axis.data(); d.mass = mass.data(); d.com = com.data(); d.inertia = inertia.data(); d.damping = damping.data(); d.spring = spring.data();
  d.rest = rest.data();
  std::vector<double> state((size_t)2 * n * B), accel((size_t)n * B), field((size_t)3 * B), cot((size_t)9 * S * B);
  if (!rd(f, state.data(), state.size()) || !rd(f, accel.data(), accel.size()) || !rd(f, field.data(), field.size()) ||
      !rd(f, cot.data(), cot.size()))
    return 2;
  fclose(f);

  void* h = shim_dyn_model(&d);
  void* set = shim_wrench_set(h, S, sbody.data(), sT.data());
  const size_t r = (size_t)3 * S * B;
  std::vector<double> out(3 * r), gs((size_t)2 * n * B), ga((size_t)n * B), gf((size_t)3 * B);
  shim_sens_forward(h, set, B, state.data(), accel.data(), field.data(), out.data(), out.data() + r, out.data() + 2 * r);
  shim_sens_vjp(h, set, B, state.data(), accel.data(), field.data(), cot.data(), cot.data() + r, cot.data() + 2 * r, gs.data(), ga.data(), gf.data(), 0);
  double sum = 0.0;
  for (double x : out) sum += x;
  for (double x : gs) sum += x;
  for (double x : ga) sum += x;
  for (double x : gf) sum += x;
  shim_wrench_set_free(set);
  shim_dyn_free(h);
  printf("sensors %d checksum %.17g\n", S, sum);
  return sum == sum ? 0 : 1;
}
