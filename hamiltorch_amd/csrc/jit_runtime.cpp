// Run-time half of the callback compiler: hipRTC -> gfx950 code object -> hipModule -> launches.
//
// hamiltorch_amd/jit/ traces a user log_prob_func (the callback contract of hamiltorch/samplers.py:272-274), writes its
// value / derivatives as straight-line device code and hands the SOURCE here; the hand-written kernels it is compiled into
// live under csrc/jit/ (hmc_callback.hip.in: the reference's sample() loop for plain HMC, samplers.py:965-1026, around that
// function; split_callback.hip.in: the same loop around a LIST of them under the split integrators, samplers.py:494-596;
// path_callback.hip.in: the per-step path of ONE leapfrog() call, samplers.py:281-302 / :494-596, around either; derivs_callback.hip.in: the derivatives the Riemannian samplers ask torch.func for, samplers.py:108, :397-398).
//
// Boundary rules as everywhere else: device pointers are the caller's, launches are enqueued on the caller's stream, nothing is
// synchronised on the launch path.  Compiling (hta_jit_compile) is host work and returns a malloc'ed code object; loading
// (hta_jit_load) creates a hipModule on the current device and reads the module's 32-byte info block back once - a
// preparation step like hta_*_prepare, outside every timed or captured region.
#include <dlfcn.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "common.hpp"
#include "jit/jit_args.h"

namespace hta {
namespace {

// ---- hipRTC through dlopen: the library loads (and everything that is not the callback compiler works) without it ----
typedef struct _hiprtcProgram* rtcProgram;
struct Rtc {
  void* h = nullptr;
  int (*create)(rtcProgram*, const char*, const char*, int, const char* const*, const char* const*) = nullptr;
  int (*compile)(rtcProgram, int, const char* const*) = nullptr;
  int (*destroy)(rtcProgram*) = nullptr;
  int (*log_size)(rtcProgram, size_t*) = nullptr;
  int (*get_log)(rtcProgram, char*) = nullptr;
  int (*code_size)(rtcProgram, size_t*) = nullptr;
  int (*get_code)(rtcProgram, char*) = nullptr;
  const char* (*err_string)(int) = nullptr;
  bool ok = false;
};

Rtc& rtc() {
  static Rtc r;
  static bool tried = false;
  if (tried) return r;
  tried = true;
  const char* names[] = {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
  for (const char* n : names) {
    r.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (r.h) break;
  }
  if (!r.h) return r;
#define HTA_RTC_SYM(field, name) *(void**)(&r.field) = dlsym(r.h, name)
  HTA_RTC_SYM(create, "hiprtcCreateProgram");
  HTA_RTC_SYM(compile, "hiprtcCompileProgram");
  HTA_RTC_SYM(destroy, "hiprtcDestroyProgram");
  HTA_RTC_SYM(log_size, "hiprtcGetProgramLogSize");
  HTA_RTC_SYM(get_log, "hiprtcGetProgramLog");
  HTA_RTC_SYM(code_size, "hiprtcGetCodeSize");
  HTA_RTC_SYM(get_code, "hiprtcGetCode");
  HTA_RTC_SYM(err_string, "hiprtcGetErrorString");
#undef HTA_RTC_SYM
  r.ok = r.create && r.compile && r.destroy && r.log_size && r.get_log && r.code_size && r.get_code;
  return r;
}

thread_local std::string g_jit_log;

struct Module {
  hipModule_t mod = nullptr;
  hipFunction_t hmc = nullptr, predraw = nullptr, derivs = nullptr, contract = nullptr, rmhmc = nullptr, split = nullptr, path = nullptr,
                rolled = nullptr;       // (rmhmc: hta_cb_rmhmc_kernel or hta_cb_rmhmc_hess_kernel, by info[4])
  int rolled_max_threads = 0;       // the launch bound hta_cb_rolled_kernel was built with
  int info[HTA_CB_INFO_WORDS] = {};
  int device = -1;
};

int check_module(const Module* m, const char* who, int D, int itemsize, int mass_kind, int set) {
  HTA_REQUIRE(m && m->mod, "%s: module is NULL", who);
  int dev = -1;
  (void)hipGetDevice(&dev);
  HTA_REQUIRE(dev == m->device, "%s: the module was loaded on device %d, the call runs on device %d", who, m->device, dev);
  HTA_REQUIRE(m->info[1] == D && m->info[2] == itemsize,
              "%s: the module was compiled for D = %d, %d-byte elements; the call has D = %d, %d-byte elements", who, m->info[1],
              m->info[2], D, itemsize);
  HTA_REQUIRE(mass_kind < 0 || m->info[3] == mass_kind, "%s: the module was compiled for mass kind %d, the call has %d", who,
              m->info[3], mass_kind);
  HTA_REQUIRE(m->info[4] == set, "%s: the module holds kernel set %d, not %d", who, m->info[4], set);
  return HTA_OK;
}

int launch(hipFunction_t fn, const char* who, int64_t C, void* args, size_t bytes, hipStream_t s, unsigned block = 64,
           unsigned per_block = 0, unsigned lds = 0) {
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
  if (per_block == 0) per_block = block;        // (the rolled kernel: several waves of a block work on the same 64 chains)
  const unsigned grid = (unsigned)((C + per_block - 1) / per_block);
  hipError_t e = hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, lds, s, nullptr, config);
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", who, hipGetErrorString(e));
    return HTA_ERR_LAUNCH;
  }
  return HTA_OK;
}

// which kernels a module of each kernel set (hta_cb_info[4]) exports, and where hta_jit_load keeps them
const struct KernelSet {
  int set;
  const char* name;
  hipFunction_t Module::*fn;
  const char* name2;          // a second kernel of the set, or NULL
  hipFunction_t Module::*fn2;
} kKernelSets[] = {
    {HTA_CB_SET_HMC, "hta_cb_hmc_kernel", &Module::hmc, "hta_cb_predraw_kernel", &Module::predraw},
    {HTA_CB_SET_DERIVS, "hta_cb_derivs_kernel", &Module::derivs, "hta_cb_contract_kernel", &Module::contract},
    {HTA_CB_SET_RMHMC, "hta_cb_rmhmc_kernel", &Module::rmhmc, nullptr, nullptr},
    {HTA_CB_SET_SPLIT, "hta_cb_split_kernel", &Module::split, nullptr, nullptr},
    {HTA_CB_SET_PATH, "hta_cb_path_kernel", &Module::path, nullptr, nullptr},          // a list (info[6] = M > 0): hta_cb_split_path_kernel
    {HTA_CB_SET_ROLLED, "hta_cb_rolled_kernel", &Module::rolled, "hta_cb_predraw_kernel", &Module::predraw},
    {HTA_CB_SET_RMHMC_HESS, "hta_cb_rmhmc_hess_kernel", &Module::rmhmc, nullptr, nullptr},
    {HTA_CB_SET_RMHMC_IMP, "hta_cb_rmhmc_imp_kernel", &Module::rmhmc, nullptr, nullptr},
    {HTA_CB_SET_RMHMC_IMP_HESS, "hta_cb_rmhmc_imp_hess_kernel", &Module::rmhmc, nullptr, nullptr},
};

const KernelSet* kernel_set(int set) {
  for (const KernelSet& k : kKernelSets)
    if (k.set == set) return &k;
  return nullptr;
}

const char* dtype_name(int itemsize) { return itemsize == 4 ? "f32" : "f64"; }
const char* split_name(int kind) { return kind == HTA_CB_SPLIT_RAND ? "rand" : kind == HTA_CB_SPLIT_KMID ? "kmid" : "symmetric"; }

// What hta_jit_hmc_sample, hta_jit_rolled_sample and hta_jit_split_sample ask of their argument block (HtaCbHmcArgs or
// HtaCbRolledArgs) before anything is launched, in three parts so that each entry point keeps the order of its checks; `who` is the
// entry point's name, `need` / `need_name` the function that sizes its workspace.
template <typename Args>
int check_args(const char* who, const Args* args, int D, int itemsize) {
  HTA_REQUIRE(args && args->cur && args->init && args->reject_count && args->C > 0 && args->L >= 0 && args->n_traj >= 0 && D > 0 &&
                  (itemsize == 4 || itemsize == 8),
              "%s: bad arguments", who);
  return HTA_OK;
}

template <typename Args>
int check_mass(const char* who, const Args* args, int mass_kind) {
  HTA_REQUIRE(mass_kind == HTA_MASS_NONE || (args->inv_mass && args->mass_factor), "%s: mass operands are NULL", who);
  return HTA_OK;
}

template <typename Args>
int check_buffers(const char* who, const Args* args, int D, int itemsize, const void* workspace, int64_t workspace_bytes,
                  int64_t (*need)(int64_t, int, int), const char* need_name) {
  HTA_REQUIRE(workspace && workspace_bytes >= need(args->C, D, itemsize), "%s: workspace of %lld bytes, %lld needed (%s)", who,
              (long long)workspace_bytes, (long long)need(args->C, D, itemsize), need_name);
  const int64_t pre_need = hta_jit_hmc_predraw_bytes(args->C, D, args->n_traj, itemsize);
  HTA_REQUIRE(!args->pre || args->pre_bytes >= pre_need, "%s: pre-draw buffer of %lld bytes, %lld needed (hta_jit_hmc_predraw_bytes)", who,
              (long long)args->pre_bytes, (long long)pre_need);
  return HTA_OK;
}

// Places the carried values in the workspace - gcur[C, D] (plain HMC: carry_grad) then lp_out[C] - and enqueues the launch: the
// pre-draw kernel (named `who_pre` in a launch error) when the block has a record buffer, then `kernel` with `block` threads per 64 chains.
template <typename Args>
int run_sample(const char* who, const char* who_pre, const Module* m, hipFunction_t kernel, Args& a, int D, int itemsize, bool carry_grad, void* workspace,
               hipStream_t s, unsigned block = 64, unsigned lds = 0) {
  a.resume = a.resume ? 1 : 0;
  a.gcur = carry_grad ? workspace : nullptr;
  a.lp_out = carry_grad ? (char*)workspace + a.C * D * itemsize : workspace;
  profile_begin(s);
  int rc = HTA_OK;
  if (a.pre) rc = launch(m->predraw, who_pre, a.C * (int64_t)a.n_traj, &a, sizeof(a), s, 256);
  if (rc == HTA_OK) rc = launch(kernel, who, a.C, &a, sizeof(a), s, block, 64, lds);
  profile_end(s);
  return rc;
}

}  // namespace
}  // namespace hta

extern "C" {

int hta_jit_available(void) { return hta::rtc().ok ? 1 : 0; }

const char* hta_jit_last_log(void) { return hta::g_jit_log.c_str(); }

int hta_jit_note_fallback(const char* reason) {
  hta::note_route("torch-evaluated callback + hmc_pieces kernels (not compiled: %s)", reason ? reason : "?");
  return HTA_OK;
}

int hta_jit_compile(const char* source, const char* name, int n_headers, const char* const* header_names,
                    const char* const* header_sources, int n_options, const char* const* options, void** code_out,
                    int64_t* code_bytes) {
  using namespace hta;
  g_jit_log.clear();
  HTA_REQUIRE(source && code_out && code_bytes && n_headers >= 0 && n_options >= 0, "hta_jit_compile: bad arguments");
  HTA_REQUIRE(n_headers == 0 || (header_names && header_sources), "hta_jit_compile: headers are NULL");
  *code_out = nullptr;
  *code_bytes = 0;
  Rtc& r = rtc();
  if (!r.ok) {
    set_error("hta_jit_compile: libhiprtc.so could not be loaded (%s)", r.h ? "symbols missing" : dlerror());
    return HTA_ERR_UNSUPPORTED;
  }
  rtcProgram prog = nullptr;
  int rc = r.create(&prog, source, name ? name : "hta_callback.hip", n_headers, header_sources, header_names);
  if (rc != 0) {
    set_error("hta_jit_compile: hiprtcCreateProgram failed (%d: %s)", rc, r.err_string ? r.err_string(rc) : "?");
    return HTA_ERR_LAUNCH;
  }
  rc = r.compile(prog, n_options, options);
  size_t ls = 0;
  if (r.log_size(prog, &ls) == 0 && ls > 1) {
    g_jit_log.resize(ls);
    (void)r.get_log(prog, &g_jit_log[0]);
  }
  if (rc != 0) {
    set_error("hta_jit_compile: hiprtcCompileProgram failed (%d: %s); hta_jit_last_log() has the compiler's messages", rc,
              r.err_string ? r.err_string(rc) : "?");
    (void)r.destroy(&prog);
    return HTA_ERR_INVALID;
  }
  size_t cs = 0;
  rc = r.code_size(prog, &cs);
  void* buf = (rc == 0 && cs > 0) ? malloc(cs) : nullptr;
  if (!buf || r.get_code(prog, (char*)buf) != 0) {
    free(buf);
    (void)r.destroy(&prog);
    set_error("hta_jit_compile: no code object (%zu bytes)", cs);
    return HTA_ERR_LAUNCH;
  }
  (void)r.destroy(&prog);
  *code_out = buf;
  *code_bytes = (int64_t)cs;
  return HTA_OK;
}

void hta_jit_free(void* code) { free(code); }

int hta_jit_load(const void* code, int64_t bytes, void** module_out) {
  using namespace hta;
  HTA_REQUIRE(code && bytes > 0 && module_out, "hta_jit_load: bad arguments");
  *module_out = nullptr;
  Module* m = new Module();
  hipError_t e = hipGetDevice(&m->device);
  if (e == hipSuccess) e = hipModuleLoadData(&m->mod, code);
  if (e != hipSuccess) {
    set_error("hta_jit_load: hipModuleLoadData: %s", hipGetErrorString(e));
    delete m;
    return HTA_ERR_LAUNCH;
  }
  hipDeviceptr_t ip = nullptr;
  size_t ib = 0;
  e = hipModuleGetGlobal(&ip, &ib, m->mod, "hta_cb_info");
  if (e == hipSuccess && ib == sizeof(m->info)) e = hipMemcpyDtoH(m->info, ip, sizeof(m->info));
  if (e != hipSuccess || ib != sizeof(m->info) || m->info[0] != HTA_CB_MAGIC) {
    set_error("hta_jit_load: the code object has no hta_cb_info block (%s)", hipGetErrorString(e));
    (void)hipModuleUnload(m->mod);
    delete m;
    return HTA_ERR_INVALID;
  }
  e = hipErrorInvalidValue;
  if (const KernelSet* k = kernel_set(m->info[4])) {
    const bool list_path = k->set == HTA_CB_SET_PATH && m->info[6] > 0;
    e = hipModuleGetFunction(&(m->*k->fn), m->mod, list_path ? "hta_cb_split_path_kernel" : k->name);
    if (e == hipSuccess && k->name2) e = hipModuleGetFunction(&(m->*k->fn2), m->mod, k->name2);
    if (e == hipSuccess && k->set == HTA_CB_SET_ROLLED)
      e = hipFuncGetAttribute(&m->rolled_max_threads, HIP_FUNC_ATTRIBUTE_MAX_THREADS_PER_BLOCK, m->rolled);
  }
  if (e != hipSuccess) {
    set_error("hta_jit_load: kernel set %d: %s", m->info[4], hipGetErrorString(e));
    (void)hipModuleUnload(m->mod);
    delete m;
    return HTA_ERR_INVALID;
  }
  *module_out = m;
  return HTA_OK;
}

int hta_jit_unload(void* module) {
  hta::Module* m = (hta::Module*)module;
  if (!m) return HTA_OK;
  if (m->mod) (void)hipModuleUnload(m->mod);
  delete m;
  return HTA_OK;
}

int hta_jit_module_info(void* module, int* info_out) {
  hta::Module* m = (hta::Module*)module;
  if (!m || !info_out) { hta::set_error("hta_jit_module_info: bad arguments"); return HTA_ERR_INVALID; }
  memcpy(info_out, m->info, sizeof(m->info));
  return HTA_OK;
}

int64_t hta_jit_hmc_workspace_bytes(int64_t C, int D, int itemsize) {
  if (C <= 0 || D <= 0 || (itemsize != 4 && itemsize != 8)) return -1;
  return C * D * itemsize + C * itemsize;       // gcur[C, D] + lp_out[C]
}

int64_t hta_jit_hmc_predraw_bytes(int64_t C, int D, int n_traj, int itemsize) {
  if (C <= 0 || D <= 0 || n_traj < 0 || (itemsize != 4 && itemsize != 8)) return -1;
  return (int64_t)n_traj * (D + 1) * C * itemsize;      // [n_traj, D + 1, C]
}

int hta_jit_hmc_sample(void* module, const HtaCbHmcArgs* args, int D, int itemsize, int mass_kind, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  using namespace hta;
  Module* m = (Module*)module;
  if (int rc = check_module(m, "hta_jit_hmc_sample", D, itemsize, mass_kind, HTA_CB_SET_HMC)) return rc;
  if (int rc = check_args("hta_jit_hmc_sample", args, D, itemsize)) return rc;
  if (int rc = check_mass("hta_jit_hmc_sample", args, mass_kind)) return rc;
  if (int rc = check_buffers("hta_jit_hmc_sample", args, D, itemsize, workspace, workspace_bytes, hta_jit_hmc_workspace_bytes,
                             "hta_jit_hmc_workspace_bytes"))
    return rc;
  if (args->n_traj == 0) return HTA_OK;
  HtaCbHmcArgs a = *args;
  a.split_kind = 0;
  note_route("hta_cb_hmc_kernel<D=%d,%s,mass=%d,nodes=%d%s>", D, dtype_name(itemsize), mass_kind, m->info[5], a.pre ? ",predrawn" : "");
  return run_sample("hta_jit_hmc_sample", "hta_jit_hmc_sample (pre-draw)", m, m->hmc, a, D, itemsize, true, workspace, (hipStream_t)stream);
}

/* Plain HMC on a callable ROLLED over its data rows (csrc/jit/rolled_callback.hip.in): a workgroup is 64 chains x args->waves waves,
 * the rows of every group divided over the waves, their partial sums added in wave order through LDS.  The arguments are checked
 * before the module is looked at: a bad wave count, a NULL table, an empty group or an LDS request beyond the bound launch nothing. */
int hta_jit_rolled_sample(void* module, const HtaCbRolledArgs* args, int D, int U, int groups, int itemsize, int mass_kind,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hta;
  Module* m = (Module*)module;
  if (int rc = check_args("hta_jit_rolled_sample", args, D, itemsize)) return rc;
  HTA_REQUIRE(U >= 0 && groups >= 1 && groups <= HTA_CB_MAX_GROUPS, "hta_jit_rolled_sample: %d groups (1 .. %d), %d uniforms", groups,
              HTA_CB_MAX_GROUPS, U);
  const int W = args->waves;
  HTA_REQUIRE(W == 1 || W == 2 || W == 4 || W == 8 || W == 16, "hta_jit_rolled_sample: %d waves per workgroup (1, 2, 4, 8 or 16)", W);
  for (int k = 0; k < groups; ++k) {
    HTA_REQUIRE(args->table[k], "hta_jit_rolled_sample: the table of group %d is NULL", k);
    HTA_REQUIRE(args->rows[k] > 0, "hta_jit_rolled_sample: group %d has %d rows", k, args->rows[k]);
  }
  const int64_t lds = (int64_t)W * 64 * (1 + D + U) * itemsize;
  HTA_REQUIRE(lds <= HTA_CB_ROLLED_LDS, "hta_jit_rolled_sample: %d waves x 64 lanes x (1 + %d + %d) values of %d bytes = %lld bytes of LDS (limit %d)",
              W, D, U, itemsize, (long long)lds, HTA_CB_ROLLED_LDS);
  if (int rc = check_mass("hta_jit_rolled_sample", args, mass_kind)) return rc;
  if (int rc = check_module(m, "hta_jit_rolled_sample", D, itemsize, mass_kind, HTA_CB_SET_ROLLED)) return rc;
  HTA_REQUIRE(m->info[6] == U && m->info[7] == groups, "hta_jit_rolled_sample: the module was compiled for %d uniforms and %d groups, the call has %d and %d",
              m->info[6], m->info[7], U, groups);
  HTA_REQUIRE(W * 64 <= m->rolled_max_threads, "hta_jit_rolled_sample: %d waves per workgroup, the kernel was built for %d", W,
              m->rolled_max_threads / 64);
  if (int rc = check_buffers("hta_jit_rolled_sample", args, D, itemsize, workspace, workspace_bytes, hta_jit_hmc_workspace_bytes,
                             "hta_jit_hmc_workspace_bytes"))
    return rc;
  if (args->n_traj == 0) return HTA_OK;
  HtaCbRolledArgs a = *args;
  a.split_kind = 0;
  int max_rows = 0;
  for (int k = 0; k < HTA_CB_MAX_GROUPS; ++k) {
    if (k >= groups) { a.table[k] = nullptr; a.rows[k] = 0; }
    if (a.rows[k] > max_rows) max_rows = a.rows[k];
  }
  note_route("hta_cb_rolled_kernel<D=%d,rows=%d,W=%d,%s,mass=%d,U=%d,groups=%d,nodes=%d%s>", D, max_rows, W, dtype_name(itemsize), mass_kind, U,
             groups, m->info[5], a.pre ? ",predrawn" : "");
  return run_sample("hta_jit_rolled_sample", "hta_jit_rolled_sample (pre-draw)", m, m->rolled, a, D, itemsize, true, workspace, (hipStream_t)stream, 64u * W, (unsigned)lds);
}

int64_t hta_jit_split_workspace_bytes(int64_t C, int D, int itemsize) {
  if (C <= 0 || D <= 0 || (itemsize != 4 && itemsize != 8)) return -1;
  return C * itemsize;                          // lp_out[C]: the split integrators carry log p only (their first kick is one subset's)
}

int hta_jit_split_sample(void* module, const HtaCbHmcArgs* args, int D, int M, int itemsize, int mass_kind, int split_kind,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hta;
  Module* m = (Module*)module;
  if (int rc = check_module(m, "hta_jit_split_sample", D, itemsize, mass_kind, HTA_CB_SET_SPLIT)) return rc;
  HTA_REQUIRE(m->info[6] == M && M >= 1 && M <= HTA_CB_MAX_SPLIT, "hta_jit_split_sample: the module was compiled for %d subsets, the call has %d",
              m->info[6], M);
  HTA_REQUIRE(split_kind == HTA_CB_SPLIT_SYMMETRIC || split_kind == HTA_CB_SPLIT_RAND || split_kind == HTA_CB_SPLIT_KMID,
              "hta_jit_split_sample: split kind %d", split_kind);
  HTA_REQUIRE(M >= 2 || split_kind == HTA_CB_SPLIT_RAND, "hta_jit_split_sample: the symmetric schemes need more than one subset (S:497-498)");
  if (int rc = check_args("hta_jit_split_sample", args, D, itemsize)) return rc;
  if (int rc = check_mass("hta_jit_split_sample", args, mass_kind)) return rc;
  HTA_REQUIRE(!args->pre, "hta_jit_split_sample: pre-drawn records are not part of the split kernel");
  if (int rc = check_buffers("hta_jit_split_sample", args, D, itemsize, workspace, workspace_bytes, hta_jit_split_workspace_bytes,
                             "hta_jit_split_workspace_bytes"))
    return rc;
  if (args->n_traj == 0) return HTA_OK;
  HtaCbHmcArgs a = *args;
  a.split_kind = split_kind;
  a.pre_bytes = 0;
  note_route("hta_cb_split_kernel<D=%d,M=%d,%s,mass=%d,kind=%s,nodes=%d>", D, M, dtype_name(itemsize), mass_kind, split_name(split_kind),
             m->info[5]);
  return run_sample("hta_jit_split_sample", nullptr, m, m->split, a, D, itemsize, false, workspace, (hipStream_t)stream);
}

/* Every step of ONE leapfrog call on a compiled callable (M == 0) or a compiled list of M callables under a split integrator
 * (csrc/jit/path_callback.hip.in): what samplers.leapfrog() returns for a (C, D) batch, in one launch. */
int hta_jit_path_leapfrog(void* module, const HtaCbPathArgs* args, int D, int M, int itemsize, int mass_kind, int split_kind,
                          void* stream) {
  using namespace hta;
  Module* m = (Module*)module;
  HTA_REQUIRE(args && args->theta0 && args->p0 && args->C > 0 && args->steps >= 0 && D > 0 && (itemsize == 4 || itemsize == 8),
              "hta_jit_path_leapfrog: bad arguments");
  HTA_REQUIRE(M >= 0 && M <= HTA_CB_MAX_SPLIT, "hta_jit_path_leapfrog: %d subsets (0 = a single callable, at most %d)", M, HTA_CB_MAX_SPLIT);
  HTA_REQUIRE(mass_kind == HTA_MASS_NONE || mass_kind == HTA_MASS_DIAG || mass_kind == HTA_MASS_FULL, "hta_jit_path_leapfrog: mass kind %d",
              mass_kind);
  HTA_REQUIRE(mass_kind == HTA_MASS_NONE || args->inv_mass, "hta_jit_path_leapfrog: inv_mass is NULL");
  if (M > 0) {
    HTA_REQUIRE(split_kind == HTA_CB_SPLIT_SYMMETRIC || split_kind == HTA_CB_SPLIT_RAND || split_kind == HTA_CB_SPLIT_KMID,
                "hta_jit_path_leapfrog: split kind %d", split_kind);
    HTA_REQUIRE(M >= 2 || split_kind == HTA_CB_SPLIT_RAND, "hta_jit_path_leapfrog: the symmetric schemes need more than one subset (S:497-498)");
  } else {
    HTA_REQUIRE(split_kind == 0, "hta_jit_path_leapfrog: a single callable has no split kind (%d)", split_kind);
  }
  HTA_REQUIRE(args->steps == 0 || (args->path_theta && args->path_p), "hta_jit_path_leapfrog: the path buffers are NULL");
  if (args->steps == 0) return HTA_OK;          // an empty path: nothing to launch, whatever the module
  if (int rc = check_module(m, "hta_jit_path_leapfrog", D, itemsize, mass_kind, HTA_CB_SET_PATH)) return rc;
  HTA_REQUIRE(m->info[6] == M, "hta_jit_path_leapfrog: the module was compiled for %d subsets, the call has %d", m->info[6], M);
  HtaCbPathArgs a = *args;
  a.split_kind = M > 0 ? split_kind : 0;
  const char* mass = mass_kind == HTA_MASS_NONE ? "none" : mass_kind == HTA_MASS_DIAG ? "diag" : "full";
  if (M > 0)
    note_route("hta_cb_split_path_kernel<D=%d,M=%d,%s,mass=%s,%s>", D, M, dtype_name(itemsize), mass, split_name(split_kind));
  else
    note_route("hta_cb_path_kernel<D=%d,%s,mass=%s>", D, dtype_name(itemsize), mass);
  profile_begin((hipStream_t)stream);
  const int rc = launch(m->path, "hta_jit_path_leapfrog", a.C, &a, sizeof(a), (hipStream_t)stream);
  profile_end((hipStream_t)stream);
  return rc;
}

int64_t hta_jit_rmhmc_workspace_bytes(int64_t C, int D, int itemsize) {
  if (C <= 0 || D <= 0 || (itemsize != 4 && itemsize != 8)) return -1;
  return C * itemsize;                          // lp_out[C]
}

/* Explicit RMHMC trajectories on a compiled callable: the module holds the soft-abs kernel (HTA_CB_SET_RMHMC) or the Metric.HESSIAN
 * one (HTA_CB_SET_RMHMC_HESS, args->alpha unread) - the launch is the same. */
int hta_jit_rmhmc_sample(void* module, const HtaCbRmhmcArgs* args, int D, int itemsize, int has_jitter, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  using namespace hta;
  Module* m = (Module*)module;
  // the module's row of kKernelSets: the set check_module asks for and the kernel's name in the route (any other module: the soft-abs row)
  const KernelSet* k = kernel_set(m && m->info[4] == HTA_CB_SET_RMHMC_HESS ? HTA_CB_SET_RMHMC_HESS : HTA_CB_SET_RMHMC);
  if (int rc = check_module(m, "hta_jit_rmhmc_sample", D, itemsize, has_jitter ? 1 : 0, k->set)) return rc;
  HTA_REQUIRE(args && args->cur && args->init && args->reject_count && args->C > 0 && args->L >= 0 && args->n_traj >= 0,
              "hta_jit_rmhmc_sample: bad arguments");
  HTA_REQUIRE(workspace && workspace_bytes >= hta_jit_rmhmc_workspace_bytes(args->C, D, itemsize),
              "hta_jit_rmhmc_sample: workspace of %lld bytes, %lld needed (hta_jit_rmhmc_workspace_bytes)", (long long)workspace_bytes,
              (long long)hta_jit_rmhmc_workspace_bytes(args->C, D, itemsize));
  if (args->n_traj == 0) return HTA_OK;
  HtaCbRmhmcArgs a = *args;
  a.lp_out = workspace;
  note_route("%s<D=%d,%s,jitter=%d,nodes=%d+%d>", k->name, D, dtype_name(itemsize), has_jitter ? 1 : 0, m->info[5], m->info[6]);
  profile_begin((hipStream_t)stream);
  const int rc = launch(m->rmhmc, "hta_jit_rmhmc_sample", a.C, &a, sizeof(a), (hipStream_t)stream);
  profile_end((hipStream_t)stream);
  return rc;
}

/* Implicit RMHMC trajectories (the generalised leapfrog with fixed-point iterations) on a compiled callable: the module holds the
 * soft-abs kernel (HTA_CB_SET_RMHMC_IMP) or the Metric.HESSIAN one (HTA_CB_SET_RMHMC_IMP_HESS, args->alpha unread). */
int hta_jit_rmhmc_implicit_sample(void* module, const HtaCbRmhmcImpArgs* args, int D, int itemsize, int has_jitter, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  using namespace hta;
  Module* m = (Module*)module;
  const KernelSet* k = kernel_set(m && m->info[4] == HTA_CB_SET_RMHMC_IMP_HESS ? HTA_CB_SET_RMHMC_IMP_HESS : HTA_CB_SET_RMHMC_IMP);
  // (the checks that need neither a module nor a device come first: they hold on a machine without a GPU too)
  HTA_REQUIRE(args && args->cur && args->init && args->reject_count && args->C > 0 && args->L >= 0 && args->n_traj >= 0,
              "hta_jit_rmhmc_implicit_sample: bad arguments");
  HTA_REQUIRE(args->max_it >= 0, "hta_jit_rmhmc_implicit_sample: max_it = %d (fixed_point_max_iterations >= 0)", args->max_it);
  HTA_REQUIRE(args->thr == args->thr, "hta_jit_rmhmc_implicit_sample: thr is NaN (fixed_point_threshold)");
  // (the jitter sub-streams of a trajectory are 32-bit positions: 2 + L (2 max_it + 2) of them)
  HTA_REQUIRE(3 + (int64_t)args->L * (2 * (int64_t)args->max_it + 2) < (int64_t)1 << 31,
              "hta_jit_rmhmc_implicit_sample: L (2 max_it + 2) = %lld sub-streams per trajectory", (long long)args->L * (2 * (long long)args->max_it + 2));
  HTA_REQUIRE(workspace && workspace_bytes >= hta_jit_rmhmc_workspace_bytes(args->C, D, itemsize),
              "hta_jit_rmhmc_implicit_sample: workspace of %lld bytes, %lld needed (hta_jit_rmhmc_workspace_bytes)", (long long)workspace_bytes,
              (long long)hta_jit_rmhmc_workspace_bytes(args->C, D, itemsize));
  if (int rc = check_module(m, "hta_jit_rmhmc_implicit_sample", D, itemsize, has_jitter ? 1 : 0, k->set)) return rc;
  if (args->n_traj == 0) return HTA_OK;
  HtaCbRmhmcImpArgs a = *args;
  a.lp_out = workspace;
  note_route("%s<D=%d,%s,jitter=%d,nodes=%d+%d>", k->name, D, dtype_name(itemsize), has_jitter ? 1 : 0, m->info[5], m->info[6]);
  profile_begin((hipStream_t)stream);
  const int rc = launch(m->rmhmc, "hta_jit_rmhmc_implicit_sample", a.C, &a, sizeof(a), (hipStream_t)stream);
  profile_end((hipStream_t)stream);
  return rc;
}

/* which: 0 = derivatives (logp / grad / neg_hess, each optional), 1 = third-order contraction (M, contract) */
int hta_jit_derivs(void* module, const HtaCbDerivArgs* args, int which, int D, int itemsize, void* stream) {
  using namespace hta;
  Module* m = (Module*)module;
  if (int rc = check_module(m, "hta_jit_derivs", D, itemsize, -1, HTA_CB_SET_DERIVS)) return rc;
  HTA_REQUIRE(args && args->theta && args->C > 0, "hta_jit_derivs: bad arguments");
  HTA_REQUIRE(which == 0 || (args->M && (args->contract || (args->upd && args->grad_in))), "hta_jit_derivs: M / contract / upd are NULL");
  HtaCbDerivArgs a = *args;
  note_route("%s<D=%d,%s,nodes=%d>", which ? "hta_cb_contract_kernel" : "hta_cb_derivs_kernel", D, dtype_name(itemsize), m->info[5]);
  return launch(which ? m->contract : m->derivs, "hta_jit_derivs", a.C, &a, sizeof(a), (hipStream_t)stream);
}

}  // extern "C"
