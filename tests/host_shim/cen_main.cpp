// Stand-alone program (its own main; never loaded into Python) for the sanitizer run of the centre-of-mass code: reads a model and inputs
// written by tests/test_centroidal_host.py, runs the host build's forward and reverse pass (cen_shim.cpp) on them and prints a checksum.
// Built by the test with -fsanitize=address,undefined.  Test harness only.
//
// Input file (text): n_bodies n_dofs B, gravity(3) dt, then per body: parent joint_type dof_offset pitch, T_pj(12), T_cj(12), axis(3), mass,
// com(3), inertia(6); then per DOF: damping spring rest; then state [2n][B], accel [n][B] and the cotangents [17][B].
#include <cstdio>
#include <cstdlib>

#include "cen_shim.cpp"

static bool rd(FILE* f, double* p, size_t k) {
  for (size_t i = 0; i < k; i++)
    if (fscanf(f, "%lf", p + i) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <input file>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  int nb = 0, n = 0, B = 0;
  if (fscanf(f, "%d %d %d", &nb, &n, &B) != 3 || nb < 1 || n < 1 || B < 1) return 2;
  nbl_model_desc d;
  std::memset(&d, 0, sizeof(d));
  d.n_bodies = nb; d.n_dofs = n;
  if (!rd(f, d.gravity, 3) || !rd(f, &d.dt, 1)) return 2;
  std::vector<int32_t> parent(nb), jt(nb), off(nb);
  std::vector<double> pitch(nb), Tpj(12 * nb), Tcj(12 * nb), axis(3 * nb), mass(nb), com(3 * nb), inertia(6 * nb), damping(n), spring(n), rest(n);
  for (int i = 0; i < nb; i++) {
    if (fscanf(f, "%d %d %d", &parent[i], &jt[i], &off[i]) != 3) return 2;
    if (!rd(f, &pitch[i], 1) || !rd(f, &Tpj[12 * i], 12) || !rd(f, &Tcj[12 * i], 12) || !rd(f, &axis[3 * i], 3) || !rd(f, &mass[i], 1) ||
        !rd(f, &com[3 * i], 3) || !rd(f, &inertia[6 * i], 6))
      return 2;
  }
  for (int j = 0; j < n; j++)
    if (!rd(f, &damping[j], 1) || !rd(f, &spring[j], 1) || !rd(f, &rest[j], 1)) return 2;
  d.parent = parent.data(); d.joint_type = jt.data(); d.dof_offset = off.data(); d.pitch = pitch.data(); d.T_pj = Tpj.data(); d.T_cj = Tcj.data();
  d.axis = axis.data(); d.mass = mass.data(); d.com = com.data(); d.inertia = inertia.data(); d.damping = damping.data(); d.spring = spring.data();
  d.rest = rest.data();
  std::vector<double> state((size_t)2 * n * B), accel((size_t)n * B), cot((size_t)17 * B);
  if (!rd(f, state.data(), state.size()) || !rd(f, accel.data(), accel.size()) || !rd(f, cot.data(), cot.size())) return 2;
  fclose(f);

  void* h = shim_dyn_model(&d);
  uint64_t masks[2];
  std::vector<double> origin(3 * CEN_MAX_BODIES);
  shim_cen_set(h, 0, nullptr, masks, nullptr, origin.data());
  std::vector<double> out((size_t)17 * B), J((size_t)3 * n * B), gs((size_t)2 * n * B), ga((size_t)n * B);
  double* o = out.data();
  const double* c = cot.data();
  shim_cen_forward(h, masks[0], masks[1], B, state.data(), accel.data(), 0, origin.data(), o, o + 3 * B, o + 6 * B, o + 9 * B, o + 15 * B, o + 16 * B, J.data());
  shim_cen_vjp(h, masks[0], masks[1], B, state.data(), accel.data(), 0, origin.data(), c, c + 3 * B, c + 6 * B, c + 9 * B, c + 15 * B, c + 16 * B, gs.data(), ga.data(), 0);
  double sum = 0.0;
  for (double x : out) sum += x;
  for (double x : J) sum += x;
  for (double x : gs) sum += x;
  for (double x : ga) sum += x;
  const double M = shim_cen_mass(h, masks[0]);
  shim_dyn_free(h);
  printf("mass %.17g checksum %.17g\n", M, sum);
  return sum == sum ? 0 : 1;
}
