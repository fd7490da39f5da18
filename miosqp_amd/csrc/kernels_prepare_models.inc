// part of engine.hip (included there, not compiled alone): the preparation of many models in ONE launch
// ------------------------------------------------------------------------------------------
// k_prepare_models: workgroup b reads entry b of a table in device memory and builds, for that model, what the host
// builds with scale_problem and pack_factor_rows: the packed rows of the panel and of the two symmetric matrices, the
// Ruiz equilibration, D, E, c, their inverses, the scaled q and the panel's values, from the raw problem, bit for bit.
// It runs ahead of the set-up launches of the same call on the group's stream; they read its output as they read the
// uploaded rows otherwise.  The arithmetic is prepare_models_body.hpp (phases between barriers; the same source runs on
// the CPU under tests/).  No workgroup waits for another.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(miosqp::prepare_models::THREADS) void k_prepare_models(const miosqp::prepare_models::IO *__restrict__ tab) {
  extern __shared__ double pm_lds[];
  SetupExecDevice x;
  miosqp::prepare_models::body(tab[blockIdx.x], pm_lds, x);
}
