// sensors.hip — gyroscope, accelerometer and magnetometer readings of a sensor set for B worlds (nbl_sensors_forward / _backward): the
// device side of Skeleton::getGyroReadings, getAccelerometerReadings and getMagnetometerReadings (Skeleton.cpp:8082-8460) and of their
// vector-Jacobian product (nimblephysics_amd/sensors.py).  The math is in sensors_dev.hpp.
//
// ONE WORLD PER LANE, like the centroidal kernels: the body constants and the entries are wave-uniform, the per-body W / V / A and their
// adjoints live in the caller's workspace laid out [body][slot][B].  No LDS, no atomics, no cross-lane operations: a world's bits do not
// depend on B or on its place in the batch.  B may be (T + 1) x worlds or rows x worlds: 64-bit world indices throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sensors_dev.hpp"

namespace NBL_NS {

constexpr int SENS_BLOCK = 64;

__global__ __launch_bounds__(SENS_BLOCK) void k_sensors(const DevBody* __restrict__ bodies, DevModel mdl, const DevKinEntry* __restrict__ entries,
                                                        const int32_t* __restrict__ path, int count, int64_t B, const double* __restrict__ state,
                                                        const double* __restrict__ accel, const double* __restrict__ field,
                                                        double* __restrict__ gyro, double* __restrict__ acc, double* __restrict__ mag,
                                                        double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * SENS_BLOCK + threadIdx.x;
  if (b >= B) return;
  sensForwardWorld(bodies, mdl.nb, mdl.n, mdl.gravity, entries, path, count, B, b, state, accel, field, gyro, acc, mag, ws);
}

__global__ __launch_bounds__(SENS_BLOCK) void k_sensors_vjp(const DevBody* __restrict__ bodies, DevModel mdl,
                                                            const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path, int count,
                                                            int64_t B, const double* __restrict__ state, const double* __restrict__ accel,
                                                            const double* __restrict__ field, const double* __restrict__ ggyro,
                                                            const double* __restrict__ gacc, const double* __restrict__ gmag,
                                                            double* __restrict__ gstate, double* __restrict__ gaccel, double* __restrict__ gfield,
                                                            int accumulate, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * SENS_BLOCK + threadIdx.x;
  if (b >= B) return;
  sensVjpWorld(bodies, mdl.nb, mdl.n, mdl.gravity, entries, path, count, B, b, state, accel, field, ggyro, gacc, gmag, gstate, gaccel, gfield,
               accumulate, ws);
}

}  // namespace NBL_NS
