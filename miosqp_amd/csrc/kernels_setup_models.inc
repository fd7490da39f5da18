// part of engine.hip (included there, not compiled alone): the dense set-up of many small models in ONE launch
// ------------------------------------------------------------------------------------------
// k_setup_models: workgroup b reads entry b of a table in device memory and builds, for that model, what
// miosqp_qp_setup builds one model at a time on a host core and with five launches: S, its LDL^T, Linv / LinvT / d2inv,
// the product form, the explicit inverse W, Kc, the guard residual, the scaled bounds and the control block.  The
// arithmetic is setup_models_body.hpp (phases between barriers; the same source runs on the CPU under tests/).
// k_setup_models_auto: the same, and for a model whose settings say rho_auto the choice of rho inside the launch -- what
// miosqp_qp_setup does with two set-ups and fifty iterations on a throw-away engine (the rho-once recipe there): the
// probing iterations on the first factor in LDS, the rule, the factor again at the chosen rho, the panel's values.  A
// kernel of its own (body_auto), so that k_setup_models stays the code it was.
// k_setup_models_large: a model beyond n + M = 192 (setup_models_large_body.hpp): only the packed triangle in LDS, Abar
// read from memory; what miosqp_qp_setup(coop = 0, resident = 0, fold = 1, pers = 0) builds -- no W, no Kc, no guard.
// k_setup_models_large_auto: the same, and for a model whose settings say rho_auto the choice of rho inside the launch
// (body_large_auto): the probing iterations on the triangle in LDS with Abar from L2, the rule, S and the factor again at
// the chosen rho, the panel's values.  A kernel of its own, so that k_setup_models_large stays the code it was.
// ------------------------------------------------------------------------------------------
struct SetupModel {
  miosqp::setup_models::IO io;  // final pointers into the call's arena
  Ctrl *ctrl;
  miosqp::setup_models::Auto au;  // read by k_setup_models_auto and k_setup_models_large_auto only
};

struct SetupExecDevice {
  template <class F>
  __device__ __forceinline__ void par(F f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
};

__device__ __forceinline__ void setup_models_reset_ctrl(Ctrl *c) {  // k_reset_ctrl
  c->done = 0;
  c->pad = 0;
  c->status = MIOSQP_QP_UNSOLVED;
  c->iter = 0;
  c->pri_res = c->dua_res = c->obj_val = 0.0;
  c->lower = __builtin_nan("");
}

__global__ __launch_bounds__(miosqp::setup_models::THREADS) void k_setup_models(const SetupModel *__restrict__ tab) {
  extern __shared__ double sm_lds[];
  const SetupModel &m = tab[blockIdx.x];
  if (threadIdx.x == 0) setup_models_reset_ctrl(m.ctrl);
  SetupExecDevice x;
  miosqp::setup_models::body(m.io, sm_lds, x);
}

// (the probing iterations keep their vectors in LDS and never touch the model's iterates in the arena, which stay at the
//  zero the arena was filled with: iterates and control block are what a fresh set-up leaves)
__global__ __launch_bounds__(miosqp::setup_models::THREADS) void k_setup_models_auto(const SetupModel *__restrict__ tab) {
  extern __shared__ double sm_lds[];
  const SetupModel &m = tab[blockIdx.x];
  if (threadIdx.x == 0) setup_models_reset_ctrl(m.ctrl);
  SetupExecDevice x;
  miosqp::setup_models::body_auto(m.io, m.au, sm_lds, x);
}

__global__ __launch_bounds__(miosqp::setup_models::THREADS) void k_setup_models_large(const SetupModel *__restrict__ tab) {
  extern __shared__ double sm_lds[];
  const SetupModel &m = tab[blockIdx.x];
  if (threadIdx.x == 0) setup_models_reset_ctrl(m.ctrl);
  SetupExecDevice x;
  miosqp::setup_models::body_large(m.io, sm_lds, x);
}

// (as in k_setup_models_auto the probing iterations keep their vectors in LDS: the model's iterates in the arena stay at
//  the zero the arena was filled with)
__global__ __launch_bounds__(miosqp::setup_models::THREADS) void k_setup_models_large_auto(const SetupModel *__restrict__ tab) {
  extern __shared__ double sm_lds[];
  const SetupModel &m = tab[blockIdx.x];
  if (threadIdx.x == 0) setup_models_reset_ctrl(m.ctrl);
  SetupExecDevice x;
  miosqp::setup_models::body_large_auto(m.io, m.au, sm_lds, x);
}
