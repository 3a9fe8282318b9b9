/* Kernel-argument blocks of the run-time compiled callback kernels: ONE definition, seen by the library (csrc/jit_runtime.cpp
 * fills them) and by the hipRTC translation unit (csrc/jit/hmc_callback.hip.in and its siblings read them).  Plain C, fixed-width fields,
 * no padding surprises: pointers first, then 8-byte scalars, then 4-byte ones. */
#ifndef HTA_JIT_ARGS_H
#define HTA_JIT_ARGS_H

#define HTA_CB_INFO_WORDS 8 /* hta_cb_info[]: {magic, D, sizeof(T), mass kind, kernel set, n_nodes, n_nodes3 (RMHMC) | M (split; path: M, 0 = one callable) | U (rolled), 0 | groups (rolled)} */
#define HTA_CB_MAGIC 0x48544131 /* "HTA1" */

/* kernel sets (hta_cb_info[4]): which entry points the module exports */
#define HTA_CB_SET_HMC 1    /* hta_cb_hmc_kernel                                            */
#define HTA_CB_SET_DERIVS 2 /* hta_cb_derivs_kernel + hta_cb_contract_kernel (Riemannian)   */
#define HTA_CB_SET_RMHMC 3  /* hta_cb_rmhmc_kernel: explicit RMHMC trajectories, D <= 16     */
#define HTA_CB_SET_SPLIT 4  /* hta_cb_split_kernel: split HMC on a LIST of callables          */
#define HTA_CB_SET_PATH 5   /* hta_cb_path_kernel | hta_cb_split_path_kernel (info[6] = M | 0): leapfrog paths */
#define HTA_CB_SET_ROLLED 6 /* hta_cb_rolled_kernel: plain HMC on a callable rolled over its data rows (info[6] = U, info[7] = groups) */
#define HTA_CB_SET_RMHMC_HESS 7 /* hta_cb_rmhmc_hess_kernel: explicit RMHMC trajectories with Metric.HESSIAN, D <= 16 (HtaCbRmhmcArgs, alpha unread) */
#define HTA_CB_SET_RMHMC_IMP 8      /* hta_cb_rmhmc_imp_kernel: implicit RMHMC trajectories (soft-abs), D <= 16 (HtaCbRmhmcImpArgs)           */
#define HTA_CB_SET_RMHMC_IMP_HESS 9 /* hta_cb_rmhmc_imp_hess_kernel: the same with Metric.HESSIAN (alpha unread)                             */

/* HTA_CB_METRIC of a generated include made for an RMHMC trajectory kernel: the values of HTA_METRIC_* in include/hamiltorch_amd.h */
#define HTA_CB_METRIC_HESSIAN 0
#define HTA_CB_METRIC_SOFTABS 1

#define HTA_CB_MAX_GROUPS 4       /* rolled groups of one callable (HtaCbRolledArgs::table / rows)                         */
#define HTA_CB_ROLLED_LDS 65536   /* bytes of dynamic LDS of one workgroup of hta_cb_rolled_kernel at most                  */

#define HTA_CB_MAX_SPLIT 16 /* subsets of a compiled list (a subset order packs into 64 bits) */
/* HtaCbHmcArgs::split_kind = HTA_SPLIT_SYMMETRIC / _RAND / _KMID of include/hamiltorch_amd.h */
#define HTA_CB_SPLIT_SYMMETRIC 0
#define HTA_CB_SPLIT_RAND 1
#define HTA_CB_SPLIT_KMID 2

/* The fields of a trajectory launch on compiled callables: HtaCbHmcArgs is this list, HtaCbRolledArgs starts with it.  ONE list, so that
 * the two cannot drift apart; the names stay flat (a.cur, a.pre) in C and in hamiltorch_amd/_abi.py. */
#define HTA_CB_HMC_FIELDS                                                                                                          \
  void* cur;               /* [C, D] current state, in / out                                                    */                 \
  const void* init;        /* [C, D] params_init (the reference's Q2 reset, samplers.py:1018)                   */                 \
  const void* inv_mass;    /* (D,) | (D,D) | NULL                                                               */                 \
  const void* mass_factor; /* sqrt(mass) (D,) | chol(mass) (D,D) lower, row-major | NULL                        */                 \
  void* samples;           /* [S, C, D] or NULL                                                                 */                 \
  int* reject_count;       /* [C]                                                                               */                 \
  void* H_old;             /* [C] of the launch's LAST trajectory, or NULL                                      */                 \
  void* H_new;             /* [C] ditto                                                                         */                 \
  unsigned char* accept;   /* [C] ditto                                                                         */                 \
  void* gcur;              /* [C, D] workspace: gradient at the current state (NULL for hta_cb_split_kernel)    */                 \
  void* lp_out;            /* [C] log p at the state the launch ended in (checked against the callback), or NULL */                \
  long long C;                                                                                                                     \
  double eps;                                                                                                                      \
  unsigned long long seed, chain_offset;                                                                                           \
  int L, n_traj, traj_offset, burn;                                                                                                \
  int resume;              /* 1: (log p, gradient) at `cur` are in the workspace from the previous launch of this run */           \
  int split_kind;          /* hta_cb_split_kernel: HTA_CB_SPLIT_*; 0 elsewhere                                  */                 \
  void* pre;               /* NULL, or [n_traj, D + 1, C] pre-drawn records of this launch (momentum after the mass factor, log u): \
                              filled by hta_cb_predraw_kernel in front of the trajectory kernel (hta_jit_hmc_predraw_bytes) */      \
  long long pre_bytes;

typedef struct HtaCbHmcArgs {
  HTA_CB_HMC_FIELDS
} HtaCbHmcArgs;

/* hta_jit_rolled_sample (csrc/jit/rolled_callback.hip.in): the fields of HtaCbHmcArgs, then the groups' tables */
typedef struct HtaCbRolledArgs {
  HTA_CB_HMC_FIELDS
  const void* table[HTA_CB_MAX_GROUPS]; /* [rows[k], slots of group k] per-row constants in the run's dtype, row-major; unused groups NULL */
  int rows[HTA_CB_MAX_GROUPS];          /* rows of group k (> 0 for the module's groups)                                             */
  int waves;               /* W: waves per workgroup of 64 chains, 1 | 2 | 4 | 8 | 16; wave w takes rows [w ceil(rows / W), ...) */
} HtaCbRolledArgs;

/* the layout the kernels, the library and hamiltorch_amd/_abi.py agree on (tests/test_jit_cpu.py holds the ctypes side) */
#ifdef __cplusplus
#define HTA_CB_LAYOUT(cond) static_assert(cond, #cond)
#else
#define HTA_CB_LAYOUT(cond) _Static_assert(cond, #cond)
#endif
HTA_CB_LAYOUT(sizeof(HtaCbHmcArgs) == 160 && sizeof(HtaCbRolledArgs) == 216);
HTA_CB_LAYOUT(__builtin_offsetof(HtaCbHmcArgs, pre) == 144 && __builtin_offsetof(HtaCbHmcArgs, pre_bytes) == 152);
HTA_CB_LAYOUT(__builtin_offsetof(HtaCbRolledArgs, pre) == 144 && __builtin_offsetof(HtaCbRolledArgs, pre_bytes) == 152);
HTA_CB_LAYOUT(__builtin_offsetof(HtaCbRolledArgs, table) == 160 && __builtin_offsetof(HtaCbRolledArgs, rows) == 192 &&
              __builtin_offsetof(HtaCbRolledArgs, waves) == 208);
#undef HTA_CB_LAYOUT

typedef struct HtaCbRmhmcArgs {
  void* cur;             /* [C, D] current state, in / out                                     */
  const void* init;      /* [C, D] params_init (Q2 reset)                                      */
  void* samples;         /* [S, C, D] or NULL                                                  */
  int* reject_count;     /* [C]                                                                */
  void* H_old;           /* [C] of the launch's last trajectory, or NULL                       */
  void* H_new;
  unsigned char* accept;
  void* lp_out;          /* [C] log p at the state the launch ended in, or NULL                */
  long long C;
  double eps, alpha, jitter, omega;
  unsigned long long seed, chain_offset;
  int L, n_traj, traj_offset, burn;
} HtaCbRmhmcArgs;

/* hta_jit_rmhmc_implicit_sample (csrc/jit/rmhmc_implicit_callback.hip.in): the generalised leapfrog with fixed-point iterations.  A block
 * of its own - the explicit kernels' kernarg block does not change: the fields of HtaCbRmhmcArgs without omega, then the fixed-point rule. */
typedef struct HtaCbRmhmcImpArgs {
  void* cur;             /* [C, D] current state, in / out                                     */
  const void* init;      /* [C, D] params_init (Q2 reset)                                      */
  void* samples;         /* [S, C, D] or NULL                                                  */
  int* reject_count;     /* [C]                                                                */
  void* H_old;           /* [C] of the launch's last trajectory, or NULL                       */
  void* H_new;
  unsigned char* accept;
  void* lp_out;          /* [C] log p at the state the launch ended in, or NULL                */
  int* iters;            /* [C] or NULL: += the fixed-point iterations the chain executed while active, both loops (tests) */
  long long C;
  double eps, alpha, jitter;
  double thr;            /* fixed_point_threshold: a chain leaves a loop once max_j (state_j - new_j)^2 < thr (compared in double) */
  unsigned long long seed, chain_offset;
  int L, n_traj, traj_offset, burn;
  int max_it;            /* fixed_point_max_iterations: the trip count of each loop at most; fixes the jitter sub-stream layout */
} HtaCbRmhmcImpArgs;

#ifdef __cplusplus
static_assert(sizeof(HtaCbRmhmcArgs) == 136, "HtaCbRmhmcArgs");
static_assert(sizeof(HtaCbRmhmcImpArgs) == 152 && __builtin_offsetof(HtaCbRmhmcImpArgs, iters) == 64 &&
                  __builtin_offsetof(HtaCbRmhmcImpArgs, C) == 72 && __builtin_offsetof(HtaCbRmhmcImpArgs, thr) == 104 &&
                  __builtin_offsetof(HtaCbRmhmcImpArgs, seed) == 112 && __builtin_offsetof(HtaCbRmhmcImpArgs, L) == 128 &&
                  __builtin_offsetof(HtaCbRmhmcImpArgs, max_it) == 144,
              "HtaCbRmhmcImpArgs");
#else
_Static_assert(sizeof(HtaCbRmhmcImpArgs) == 152, "HtaCbRmhmcImpArgs");
#endif

/* hta_jit_path_leapfrog (csrc/jit/path_callback.hip.in): every step of one leapfrog call, nothing drawn, nothing decided */
typedef struct HtaCbPathArgs {
  const void* theta0;   /* [C, D] start points                                                        */
  const void* p0;       /* [C, D] start momenta                                                       */
  const void* inv_mass; /* (D,) | (D,D) | NULL                                                        */
  void* path_theta;     /* [steps, C, D]: theta after every step                                      */
  void* path_p;         /* [steps, C, D]: p after every step (plain HMC: the last row after S:302)    */
  void* lp_end;         /* [C] log p at the end points (a list: the sum over the subsets), or NULL    */
  long long C;
  double eps;
  unsigned long long seed; /* SPLITTING_RAND: the subset order is hta::split_permutation(seed, 0, M)  */
  int steps;
  int split_kind;       /* hta_cb_split_path_kernel: HTA_CB_SPLIT_*; 0 for a single callable          */
} HtaCbPathArgs;

typedef struct HtaCbDerivArgs {
  const void* theta; /* [C, D]                                              */
  void* logp;        /* [C] or NULL                                         */
  void* grad;        /* [C, D] or NULL                                      */
  void* neg_hess;    /* [C, D, D] or NULL: -Hessian of log p (samplers.py:108) */
  const void* M;     /* [C, D, D] (contract kernel)                         */
  void* contract;    /* [C, D] or NULL: c_i = d_i < Hess log p, M >, M held fixed */
  void* upd;         /* [C, D] or NULL: upd += coef * (grad_in + c) - the momentum update of S:395-398 fused into the contraction */
  const void* grad_in; /* [C, D]: gradient of log p at theta (with upd)      */
  double coef;
  long long C;
} HtaCbDerivArgs;

#endif
