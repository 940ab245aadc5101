// Pose-graph optimisation — C-ABI entry points msfl_graph_*: poses on the device, the graph's structure on the host, Ceres' trust-region
// loop enqueued as a fixed launch pattern per LM iteration.  Included at the end of msfl_api.hip (shares DevBuf, PinRing, PinBuf and
// the helper macros); kernels: msfl_graph.cuh.  The object owns its stream and all its memory, like msfl_places.

#include "msfl_graph.cuh"   // includes msfl_graph_host.h: GraphStructure, graph_build_structure, graph_levels

static_assert(sizeof(msfl_graph_edge) == 80 && sizeof(msfl_graph_fix) == 48 && sizeof(msfl_graph_summary) == 48, "graph record layout");
static_assert(sizeof(msfl_graph_edge_info) == 352 && sizeof(msfl_graph_fix_info) == 112, "information factor record layout");
static_assert(sizeof(GraphState) % 8 == 0, "the trace follows the state record");
static_assert(sizeof(msfl_graph_marginals_summary) == 32 && sizeof(msfl_graph_marginals_options) == 24, "marginals record layout");
static_assert(sizeof(GraphMargCol) == 32 && sizeof(GraphMargState) == 16, "marginals state records, read back as they are");
static_assert(sizeof(msfl_graph_loss) == 16, "loss record layout");
static_assert(MSFL_GRAPH_LOSS_DEFAULT == kGraphLossDefault && MSFL_GRAPH_LOSS_NONE == kGraphLossNone && MSFL_GRAPH_LOSS_HUBER == kGraphLossHuber &&
              MSFL_GRAPH_LOSS_SOFT_L_ONE == kGraphLossSoftLOne && MSFL_GRAPH_LOSS_CAUCHY == kGraphLossCauchy &&
              MSFL_GRAPH_LOSS_GEMAN_MCCLURE == kGraphLossGemanMcClure, "the loss kinds of msfl_graph_host.h are the header's");

struct msfl_graph_s {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  msfl_graph_config cfg{};
  std::string last_error;
  int n_nodes = 0;
  std::vector<unsigned char> fixed;
  std::vector<msfl_graph_edge> edges;
  std::vector<msfl_graph_fix> fixes;
  std::vector<msfl_graph_edge_info> edges_info;    // count against max_edges together with `edges`
  std::vector<msfl_graph_fix_info> fixes_info;     // count against max_fixes together with `fixes`
  bool dirty = true;             // the structure changed since the device copy was built
  GraphStructure gs;
  GraphLevels lv{};
  GraphDev dev{};
  std::vector<int> tr_accepted;  // the last optimize's trace
  std::vector<double> tr_cost;
  DevBuf x, cand;                // double[max_nodes x 7]
  DevBuf ints, data, work;       // structure, factor data, everything the solve works in
  DevBuf linfo;                  // double[information factors x 36]: their L; allocated by the first call that adds one
  DevBuf chi;                    // msfl_graph_factor_chi2's / msfl_graph_factor_weights' result before it goes to the host
  // msfl_graph_set_losses; nothing of it exists before the first call
  bool has_losses = false;       // from the first call to the next clear: every factor has a record, DEFAULT unless set
  bool loss_dirty = false;       // records changed since the device copy was built
  std::vector<msfl_graph_loss> losses[4];   // per factor kind, in the order added
  DevBuf loss;                   // double a[factors] | int kind[factors], in the factor numbering
  GraphLossDev loss_dev{};
  DevBuf state;                  // GraphState, double[max_iter] candidate costs, one double (msfl_graph_cost), int[max_iter] accept list
  PinRing pin;
  PinBuf readback;
  // msfl_graph_marginals; all of it allocated by the first call
  DevBuf marg_work;              // the column blocks of one chunk, the CG partials, the pivot partials
  DevBuf marg_state;             // GraphState (zero: the reused kernels' `done`), GraphMargState, GraphMargCol[6 x column nodes]
  DevBuf marg_ints;              // free index per column node | per pair: free index of a, column index of b
  DevBuf marg_out;               // the blocks before they go to the host
  PinBuf marg_read;
};

namespace {

msfl_status fail(msfl_graph* g, msfl_status s, const std::string& msg) {
  if (g) g->last_error = msg;
  return s;
}

msfl_status enter(msfl_graph* g) {
  if (!g) return MSFL_BAD_ARG;
  HIPCHK(g, hipSetDevice(g->device));
  return MSFL_OK;
}

bool graph_config_ok(const msfl_graph_config& c) {
  const double d[] = {c.huber_delta, c.initial_trust_region_radius, c.max_trust_region_radius, c.min_trust_region_radius, c.min_relative_decrease,
                      c.min_lm_diagonal, c.max_lm_diagonal, c.function_tolerance, c.gradient_tolerance, c.parameter_tolerance, c.cg_tolerance};
  for (double v : d)
    if (!std::isfinite(v) || v < 0.0) return false;
  return c.max_nodes >= 1 && c.max_edges >= 0 && c.max_fixes >= 0 && c.max_num_iterations >= 0 && c.max_num_iterations <= 10000 &&
         c.max_consecutive_invalid_steps >= 1 && c.max_cg_iterations >= 0 && c.initial_trust_region_radius > 0.0 &&
         c.min_lm_diagonal <= c.max_lm_diagonal;
}

GraphOpt graph_opt(const msfl_graph_config& c) {
  GraphOpt o{};
  o.max_iter = c.max_num_iterations; o.max_invalid = c.max_consecutive_invalid_steps; o.jacobi = c.jacobi_scaling;
  o.huber = c.huber_delta; o.radius0 = c.initial_trust_region_radius; o.radius_max = c.max_trust_region_radius;
  o.radius_min = c.min_trust_region_radius; o.min_rel = c.min_relative_decrease; o.lm_min = c.min_lm_diagonal; o.lm_max = c.max_lm_diagonal;
  o.ftol = c.function_tolerance; o.gtol = c.gradient_tolerance; o.ptol = c.parameter_tolerance; o.cg_tol = c.cg_tolerance;
  return o;
}

bool graph_pose_ok(const double* p) {
  for (int c = 0; c < 7; c++)
    if (!std::isfinite(p[c])) return false;
  return p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6] > 0.0;
}

size_t graph_state_bytes(const msfl_graph* g) {
  const size_t n = (size_t)std::max(1, g->cfg.max_num_iterations);   // state | double[n] candidate costs | one double (msfl_graph_cost) | int[n] accept list
  return sizeof(GraphState) + (n + 1) * sizeof(double) + ((n + 1) & ~size_t(1)) * sizeof(int);
}

// hands out consecutive pieces of a work area
struct GraphCarve {
  double* w;
  double* operator()(size_t n) { double* p = w; w += n; return p; }
};

// Builds the device copy of the structure and carves the work area; nothing to do while the structure is unchanged.
msfl_status graph_prepare_losses(msfl_graph* g);
msfl_status graph_prepare(msfl_graph* g) {
  if (!g->dirty) return graph_prepare_losses(g);
  hipStream_t st = g->stream;
  const int ne = (int)g->edges.size(), nx = (int)g->fixes.size(), nei = (int)g->edges_info.size(), nxi = (int)g->fixes_info.size();
  const int np = ne + nx, ni = nei + nxi, nf = np + ni;      // factor numbering: edges, fixes, information edges, information fixes
  std::vector<int> ij(2 * (size_t)nf);
  std::vector<double> data(9 * (size_t)std::max(1, nf));
  for (int k = 0; k < ne; k++) {
    const msfl_graph_edge& e = g->edges[k];
    ij[2 * k] = e.i; ij[2 * k + 1] = e.j;
    double* d = data.data() + 9 * (size_t)k;
    for (int c = 0; c < 7; c++) d[c] = e.z[c];
    d[7] = e.sr; d[8] = e.st;
  }
  for (int k = 0; k < nx; k++) {
    const msfl_graph_fix& f = g->fixes[k];
    ij[2 * (ne + k)] = f.i; ij[2 * (ne + k) + 1] = f.j;
    double* d = data.data() + 9 * (size_t)(ne + k);
    d[0] = f.t; d[1] = f.p[0]; d[2] = f.p[1]; d[3] = f.p[2]; d[4] = f.st; d[5] = d[6] = d[7] = d[8] = 0.0;
  }
  std::vector<double> linfo(36 * (size_t)ni, 0.0);
  for (int k = 0; k < nei; k++) {
    const msfl_graph_edge_info& e = g->edges_info[k];
    ij[2 * (np + k)] = e.i; ij[2 * (np + k) + 1] = e.j;
    std::copy(e.z, e.z + 7, data.data() + 9 * (size_t)(np + k));
    std::copy(e.sqrt_information, e.sqrt_information + 36, linfo.data() + 36 * (size_t)k);
  }
  for (int k = 0; k < nxi; k++) {
    const msfl_graph_fix_info& f = g->fixes_info[k];
    ij[2 * (np + nei + k)] = f.i; ij[2 * (np + nei + k) + 1] = f.j;
    double* d = data.data() + 9 * (size_t)(np + nei + k);
    d[0] = f.t; d[1] = f.p[0]; d[2] = f.p[1]; d[3] = f.p[2];
    std::copy(f.sqrt_information, f.sqrt_information + 9, linfo.data() + 36 * (size_t)(nei + k));
  }
  GraphStructure& s = g->gs;
  graph_build_structure(g->n_nodes, g->fixed.data(), ij, &s);
  const int F = s.n_free, N = g->n_nodes;
  g->lv = graph_levels(std::max(1, F));
  // ints: free_of | node_of | adj_off | adj | ladj_off | ladj | fac_ij
  std::vector<int> ints;
  size_t at[7]; int q = 0;
  for (const std::vector<int>* v : {&s.free_of, &s.node_of, &s.adj_off, &s.adj, &s.ladj_off, &s.ladj, &s.fac_ij}) {
    at[q++] = ints.size();
    ints.insert(ints.end(), v->begin(), v->end());
  }
  ints.push_back(0);
  HIPCHK(g, g->ints.reserve(ints.size() * sizeof(int)));
  HIPCHK(g, g->pin.upload(g->ints.p, ints.data(), ints.size() * sizeof(int), st));
  HIPCHK(g, g->data.reserve(data.size() * sizeof(double)));
  HIPCHK(g, g->pin.upload(g->data.p, data.data(), data.size() * sizeof(double), st));
  if (ni) {
    HIPCHK(g, g->linfo.reserve(linfo.size() * sizeof(double)));
    HIPCHK(g, g->pin.upload(g->linfo.p, linfo.data(), linfo.size() * sizeof(double), st));
  }
  const GraphLevels& v = g->lv;
  const size_t blocks = (size_t)v.off[v.count - 1] + 1, inv = (size_t)v.ioff[v.count - 1] + 1, Fz = (size_t)std::max(1, F), nfz = (size_t)std::max(1, nf);
  const size_t n_part = (Fz + kGraphVec - 1) / kGraphVec;
  const size_t want = nfz * (kGraphJ + 2) + Fz * (36 + 36 + 6 + 6 + 3) + blocks * (36 + 36 + 6 + 6) + inv * 36 + Fz * 6 * 7 + 2 * n_part;
  HIPCHK(g, g->work.reserve(want * sizeof(double)));
  GraphDev& d = g->dev;
  d = GraphDev{};
  d.n_nodes = N; d.n_free = F; d.n_edges = ne; d.n_factors = nf; d.n_plain = np; d.n_einfo = nei;
  d.fac_L = g->linfo.as<double>();
  const int* ip = g->ints.as<int>();
  d.free_of = ip + at[0]; d.node_of = ip + at[1]; d.adj_off = ip + at[2]; d.adj = ip + at[3]; d.ladj_off = ip + at[4]; d.ladj = ip + at[5];
  d.fac_ij = ip + at[6];
  d.fac_data = g->data.as<double>();
  d.x = g->x.as<double>(); d.cand = g->cand.as<double>();
  GraphCarve carve{g->work.as<double>()};
  d.J = carve(nfz * kGraphJ); d.fcost = carve(nfz); d.fmodel = carve(nfz);
  d.H = carve(Fz * 36); d.Lb = carve(Fz * 36); d.g = carve(Fz * 6); d.scale = carve(Fz * 6);
  d.nxx = carve(Fz); d.ngmax = carve(Fz); d.nstep = carve(Fz);
  d.D = carve(blocks * 36); d.L = carve(blocks * 36); d.rhs = carve(blocks * 6); d.sol = carve(blocks * 6);
  d.Dinv = carve(inv * 36);
  d.b = carve(Fz * 6); d.xs = carve(Fz * 6); d.r = carve(Fz * 6); d.z = carve(Fz * 6); d.p[0] = carve(Fz * 6); d.p[1] = carve(Fz * 6); d.q = carve(Fz * 6);
  d.part = carve(2 * n_part);
  char* sp = g->state.as<char>();
  d.st = reinterpret_cast<GraphState*>(sp);
  d.tr_cost = reinterpret_cast<double*>(sp + sizeof(GraphState));
  d.tr_accepted = reinterpret_cast<int*>(sp + sizeof(GraphState) + ((size_t)std::max(1, g->cfg.max_num_iterations) + 1) * sizeof(double));
  g->dirty = false;
  g->loss_dirty = g->has_losses;
  return graph_prepare_losses(g);
}

// the device copy of the loss records, in the factor numbering; nothing to do for a graph without records or while they are unchanged
msfl_status graph_prepare_losses(msfl_graph* g) {
  if (!g->loss_dirty) return MSFL_OK;
  const size_t nf = (size_t)g->dev.n_factors, nfz = std::max<size_t>(1, nf);
  std::vector<double> a(nfz, 0.0);
  std::vector<int> kind(nfz, MSFL_GRAPH_LOSS_DEFAULT);
  size_t k = 0;
  for (const std::vector<msfl_graph_loss>& v : g->losses)
    for (const msfl_graph_loss& l : v) { a[k] = l.a; kind[k] = l.kind; k++; }
  HIPCHK(g, g->loss.reserve(nfz * (sizeof(double) + sizeof(int))));
  HIPCHK(g, g->pin.upload(g->loss.p, a.data(), nfz * sizeof(double), g->stream));
  HIPCHK(g, g->pin.upload(g->loss.as<double>() + nfz, kind.data(), nfz * sizeof(int), g->stream));
  g->loss_dev.a = g->loss.as<double>();
  g->loss_dev.kind = reinterpret_cast<const int*>(g->loss.as<double>() + nfz);
  g->loss_dirty = false;
  return MSFL_OK;
}

// one lane per item; ny: the grid's y (the marginals' column nodes)
template <class K, class... A>
void graph_launch_y(hipStream_t st, K kernel, int items, int block, int ny, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)std::max(1, div_up(items, block)), (unsigned)ny), dim3(block), 0, st, args...);
}
template <class K, class... A>
void graph_launch(hipStream_t st, K kernel, int items, int block, A... args) {
  graph_launch_y(st, kernel, items, block, 1, args...);
}

// The pieces of the launch pattern that msfl_graph_optimize and msfl_graph_marginals share.  They take the stream and the GraphDev to
// run on: the marginals run on a copy whose `st` is a state record of their own.

// the factor kernels: the plain kinds and, only when the graph holds one, the information kinds
// `L` is null for a graph without loss records (the kernels there always were), else the per-factor arrays (their siblings)
void graph_enqueue_linearize(hipStream_t st, const GraphDev& d, double huber, const GraphLossDev* L) {
  const int ni = d.n_factors - d.n_plain;
  if (!L) {
    if (d.n_plain) graph_launch(st, graph_linearize_kernel<>, d.n_plain, kGraphBlock, d, huber);
    if (ni) graph_launch(st, graph_linearize_info_kernel<>, ni, kGraphBlock, d, huber);
    return;
  }
  if (d.n_plain) graph_launch(st, graph_linearize_kernel<GraphLossDev>, d.n_plain, kGraphBlock, d, huber, *L);
  if (ni) graph_launch(st, graph_linearize_info_kernel<GraphLossDev>, ni, kGraphBlock, d, huber, *L);
}
template <bool kModel>
void graph_enqueue_cost(hipStream_t st, const GraphDev& d, const double* x, double huber, const GraphLossDev* L) {
  const int ni = d.n_factors - d.n_plain;
  if (!L) {
    if (d.n_plain) graph_launch(st, graph_cost_kernel<kModel>, d.n_plain, kGraphBlock, d, x, huber);
    if (ni) graph_launch(st, graph_cost_info_kernel<kModel>, ni, kGraphBlock, d, x, huber);
    return;
  }
  if (d.n_plain) graph_launch(st, graph_cost_kernel<kModel, GraphLossDev>, d.n_plain, kGraphBlock, d, x, huber, *L);
  if (ni) graph_launch(st, graph_cost_info_kernel<kModel, GraphLossDev>, ni, kGraphBlock, d, x, huber, *L);
}
const GraphLossDev* graph_losses(const msfl_graph* g) { return g->has_losses ? &g->loss_dev : nullptr; }

// workgroups of the invert launch of level l: with kPivot each leaves one partial minimum in M.piv
int graph_invert_groups(const GraphLevels& v, int l) { return std::max(1, div_up(v.n[l] / 2, kGraphBlock)); }

// the factor half of the cyclic reduction of d.D / d.L; with kPivot also the pivot test into M.st (M is not looked at otherwise)
template <bool kPivot>
void graph_enqueue_factor(hipStream_t st, const GraphDev& d, const GraphLevels& v, const GraphMarg& M, double min_ratio) {
  int n_piv = 0;
  for (int l = 0; l < v.tail; l++) {
    graph_launch(st, graph_cr_invert_kernel<kPivot>, v.n[l] / 2, kGraphBlock, d, v, l, M, n_piv);
    n_piv += graph_invert_groups(v, l);
    graph_launch(st, graph_cr_reduce_kernel, v.n[l + 1], kGraphBlock, d, v, l);
  }
  graph_launch(st, graph_cr_factor_tail_kernel<kPivot>, 1, kGraphVec, d, v, M, n_piv, min_ratio);
}

// x0 = T^-1 y0, the right-hand-side half of the cyclic reduction, for the columns of `cols` over a grid of ny in y
template <class C>
void graph_enqueue_solve(hipStream_t st, const GraphDev& d, const GraphLevels& v, int ny, const C& cols) {
  for (int l = 0; l < v.tail; l++) graph_launch_y(st, graph_cr_rhs_kernel<C>, v.n[l + 1], C::kLanes, ny, d, v, l, cols);
  graph_launch_y(st, graph_cr_tail_kernel<C>, 1, kGraphVec, ny, d, v, cols);
  for (int l = v.tail - 1; l >= 0; l--) graph_launch_y(st, graph_cr_back_kernel<C>, v.n[l], C::kLanes, ny, d, v, l, cols);
}

msfl_status graph_read_state(msfl_graph* g, GraphState* out) {
  HIPCHK(g, hipMemcpyAsync(g->readback.p, g->state.p, graph_state_bytes(g), hipMemcpyDeviceToHost, g->stream));
  HIPCHK(g, hipStreamSynchronize(g->stream));
  std::memcpy(out, g->readback.p, sizeof(GraphState));
  return MSFL_OK;
}

// The checked append behind the four msfl_graph_add_*: nothing is stored unless the whole batch passes.  `held` counts what already
// stands against `cap` (a kind and its information sibling together), `fits` is the text after "<who>: " when the batch does not fit,
// `ok` the per-record test and `bad` the text when it fails; an information kind also gets room for its L matrices on the device.
template <class R, class Ok>
msfl_status graph_append(msfl_graph* g, const std::string& who, std::vector<R>& to, const R* recs, int n, size_t held, int cap, const char* fits,
                         Ok ok, const char* bad, bool information, int kind) {
  msfl_status s = enter(g); if (s) return s;
  if (n < 0 || (n > 0 && !recs)) return fail(g, MSFL_BAD_ARG, who + ": null array or negative count");
  if ((long long)held + n > cap) return fail(g, MSFL_CAPACITY, who + ": " + fits + "; nothing added");
  for (int k = 0; k < n; k++) {
    const R& r = recs[k];
    if (r.i < 0 || r.j < 0 || r.i >= g->n_nodes || r.j >= g->n_nodes || r.i == r.j)
      return fail(g, MSFL_BAD_ARG, who + ": a node index out of range or i == j; nothing added");
    if (!ok(r)) return fail(g, MSFL_BAD_ARG, who + ": " + bad + "; nothing added");
  }
  if (n == 0) return MSFL_OK;
  if (information) HIPCHK(g, g->linfo.reserve(36 * sizeof(double) * (g->edges_info.size() + g->fixes_info.size() + (size_t)n)));
  to.insert(to.end(), recs, recs + n);
  if (g->has_losses) g->losses[kind].resize(to.size(), msfl_graph_loss{MSFL_GRAPH_LOSS_DEFAULT, 0, 0.0});
  g->dirty = true;
  return MSFL_OK;
}

// kind, first, n name factors the graph holds; *k0: the first one's place in the factor numbering
bool graph_factor_range(const msfl_graph* g, int kind, int first, int n, int* k0) {
  const int count[4] = {(int)g->edges.size(), (int)g->fixes.size(), (int)g->edges_info.size(), (int)g->fixes_info.size()};
  if (kind < 0 || kind > 3 || first < 0 || n < 0 || (long long)first + n > count[kind]) return false;
  *k0 = first;
  for (int c = 0; c < kind; c++) *k0 += count[c];
  return true;
}

bool graph_fix_point_ok(double t, const double* p) {
  return std::isfinite(t) && std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && t >= 0.0 && t <= 1.0;
}

}  // namespace

extern "C" {

void msfl_graph_default_config(msfl_graph_config* c) {
  if (!c) return;
  c->max_nodes = 16384; c->max_edges = 32768; c->max_fixes = 16384;
  c->max_num_iterations = 10; c->max_consecutive_invalid_steps = 5; c->jacobi_scaling = 1; c->max_cg_iterations = 0; c->reserved = 0;
  c->huber_delta = 1.0;
  c->initial_trust_region_radius = 1e4; c->max_trust_region_radius = 1e16; c->min_trust_region_radius = 1e-32;
  c->min_relative_decrease = 1e-3; c->min_lm_diagonal = 1e-6; c->max_lm_diagonal = 1e32;
  c->function_tolerance = 1e-6; c->gradient_tolerance = 1e-10; c->parameter_tolerance = 1e-8;
  c->cg_tolerance = 1e-12;
}

msfl_status msfl_graph_create(const msfl_graph_config* cfg, int device, msfl_graph** out) {
  if (!out) return MSFL_BAD_ARG;
  *out = nullptr;
  msfl_graph_config c;
  if (cfg) c = *cfg; else msfl_graph_default_config(&c);
  if (!graph_config_ok(c)) return MSFL_BAD_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MSFL_HIP_ERROR;   // no GPU: fail loudly, no fallback
  if (device < 0 || device >= ndev) return MSFL_BAD_ARG;
  msfl_graph* g = new msfl_graph_s();
  g->device = device; g->cfg = c;
  const size_t pose_bytes = (size_t)c.max_nodes * 7 * sizeof(double);
  bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&g->own_stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && g->x.reserve(pose_bytes) == hipSuccess && g->cand.reserve(pose_bytes) == hipSuccess &&
       g->state.reserve(graph_state_bytes(g)) == hipSuccess && g->readback.reserve(std::max(graph_state_bytes(g), (size_t)4096)) == hipSuccess;
  if (!ok) { msfl_graph_destroy(g); return MSFL_HIP_ERROR; }
  g->stream = g->own_stream;
  *out = g;
  return MSFL_OK;
}

void msfl_graph_destroy(msfl_graph* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  if (g->own_stream) (void)hipStreamDestroy(g->own_stream);
  delete g;
}

msfl_status msfl_graph_set_stream(msfl_graph* g, void* hip_stream) {
  msfl_status s = enter(g); if (s) return s;
  HIPCHK(g, hipStreamSynchronize(g->stream));
  g->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return MSFL_OK;
}

msfl_status msfl_graph_synchronize(msfl_graph* g) {
  msfl_status s = enter(g); if (s) return s;
  HIPCHK(g, hipStreamSynchronize(g->stream));
  return MSFL_OK;
}

const char* msfl_graph_last_error(const msfl_graph* g) { return g ? g->last_error.c_str() : "null graph object"; }

int msfl_graph_num_nodes(const msfl_graph* g) { return g ? g->n_nodes : 0; }

msfl_status msfl_graph_clear(msfl_graph* g) {
  msfl_status s = enter(g); if (s) return s;
  HIPCHK(g, hipStreamSynchronize(g->stream));
  g->n_nodes = 0; g->fixed.clear(); g->edges.clear(); g->fixes.clear(); g->edges_info.clear(); g->fixes_info.clear(); g->tr_accepted.clear(); g->tr_cost.clear();
  for (std::vector<msfl_graph_loss>& v : g->losses) v.clear();
  g->has_losses = false; g->loss_dirty = false;
  g->dirty = true;
  return MSFL_OK;
}

// poses in host or device memory are checked on the host before anything is stored (a device array is read back first)
static msfl_status graph_store_poses(msfl_graph* g, const char* who, const double* poses, int first, int n, msfl_mem mem) {
  const std::string w(who);
  std::vector<double> host;
  const double* hp = poses;
  if (mem == MSFL_MEM_DEVICE) {
    host.resize((size_t)n * 7);
    HIPCHK(g, hipStreamSynchronize(g->stream));
    HIPCHK(g, hipMemcpy(host.data(), poses, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    hp = host.data();
  }
  for (int i = 0; i < n; i++)
    if (!graph_pose_ok(hp + 7 * (size_t)i)) return fail(g, MSFL_BAD_ARG, w + ": a pose with a non-finite value or a zero quaternion; nothing stored");
  double* dst = g->x.as<double>() + (size_t)first * 7;
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(g, g->pin.upload(dst, poses, (size_t)n * 7 * sizeof(double), g->stream));
  } else {
    HIPCHK(g, hipMemcpyAsync(dst, poses, (size_t)n * 7 * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
  }
  return MSFL_OK;
}

msfl_status msfl_graph_add_nodes(msfl_graph* g, const double* poses, int n, msfl_mem mem, int* first_index) {
  msfl_status s = enter(g); if (s) return s;
  if (n < 0 || (n > 0 && !poses) || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE))
    return fail(g, MSFL_BAD_ARG, "msfl_graph_add_nodes: null array, negative count or unknown memory kind");
  if ((long long)g->n_nodes + n > g->cfg.max_nodes) return fail(g, MSFL_CAPACITY, "msfl_graph_add_nodes: the batch does not fit max_nodes; nothing added");
  if (first_index) *first_index = g->n_nodes;
  if (n == 0) return MSFL_OK;
  s = graph_store_poses(g, "msfl_graph_add_nodes", poses, g->n_nodes, n, mem); if (s) return s;
  g->n_nodes += n; g->fixed.resize((size_t)g->n_nodes, 0);
  g->dirty = true;
  return MSFL_OK;
}

msfl_status msfl_graph_add_edges(msfl_graph* g, const msfl_graph_edge* edges, int n) {
  if (!g) return MSFL_BAD_ARG;
  return graph_append(g, "msfl_graph_add_edges", g->edges, edges, n, g->edges.size() + g->edges_info.size(), g->cfg.max_edges,
                      "the batch does not fit max_edges",
                      [](const msfl_graph_edge& e) { return graph_pose_ok(e.z) && std::isfinite(e.sr) && std::isfinite(e.st) && e.sr > 0.0 && e.st > 0.0; },
                      "a non-finite value, a zero quaternion or sr, st <= 0", false, MSFL_GRAPH_FACTOR_EDGE);
}

msfl_status msfl_graph_add_fixes(msfl_graph* g, const msfl_graph_fix* fixes, int n) {
  if (!g) return MSFL_BAD_ARG;
  return graph_append(g, "msfl_graph_add_fixes", g->fixes, fixes, n, g->fixes.size() + g->fixes_info.size(), g->cfg.max_fixes,
                      "the batch does not fit max_fixes",
                      [](const msfl_graph_fix& f) { return graph_fix_point_ok(f.t, f.p) && std::isfinite(f.st) && f.st > 0.0; },
                      "a non-finite value, st <= 0 or t outside [0, 1]", false, MSFL_GRAPH_FACTOR_FIX);
}

msfl_status msfl_graph_add_edges_info(msfl_graph* g, const msfl_graph_edge_info* edges, int n) {
  if (!g) return MSFL_BAD_ARG;
  return graph_append(g, "msfl_graph_add_edges_info", g->edges_info, edges, n, g->edges.size() + g->edges_info.size(), g->cfg.max_edges,
                      "plain and information edges together do not fit max_edges",
                      [](const msfl_graph_edge_info& e) { return graph_pose_ok(e.z) && graph_sqrt_information_ok(e.sqrt_information, 36); },
                      "a non-finite value, a zero quaternion or an all-zero sqrt_information", true, MSFL_GRAPH_FACTOR_EDGE_INFO);
}

msfl_status msfl_graph_add_fixes_info(msfl_graph* g, const msfl_graph_fix_info* fixes, int n) {
  if (!g) return MSFL_BAD_ARG;
  return graph_append(g, "msfl_graph_add_fixes_info", g->fixes_info, fixes, n, g->fixes.size() + g->fixes_info.size(), g->cfg.max_fixes,
                      "plain and information fixes together do not fit max_fixes",
                      [](const msfl_graph_fix_info& f) { return graph_fix_point_ok(f.t, f.p) && graph_sqrt_information_ok(f.sqrt_information, 9); },
                      "a non-finite value, t outside [0, 1] or an all-zero sqrt_information", true, MSFL_GRAPH_FACTOR_FIX_INFO);
}

// pure host arithmetic (msfl_graph_host.h): no graph object, no GPU call
msfl_status msfl_graph_edge_from_uncertainty(int i, int j, const double* pose_i, const double* pose_j, const msfl_match_uncertainty* unc,
                                             double scale, msfl_graph_edge_info* out) {
  if (!pose_i || !pose_j || !unc || !out || i < 0 || j < 0 || i == j || !unc->valid) return MSFL_BAD_ARG;
  msfl_graph_edge_info e{};
  e.i = i; e.j = j;
  if (!graph_edge_from_eigen(pose_i, pose_j, unc->eigenvalues, unc->eigenvectors, unc->n_degenerate, scale, e.z, e.sqrt_information))
    return MSFL_BAD_ARG;
  *out = e;
  return MSFL_OK;
}

msfl_status msfl_graph_fix_from_covariance(int i, int j, double t, const double* p, const double* covariance, msfl_graph_fix_info* out) {
  if (!p || !covariance || !out || i < 0 || j < 0 || i == j || !(t >= 0.0 && t <= 1.0) || !graph_all_finite(p, 3)) return MSFL_BAD_ARG;
  msfl_graph_fix_info f{};
  f.i = i; f.j = j; f.t = t; f.p[0] = p[0]; f.p[1] = p[1]; f.p[2] = p[2];
  if (!graph_fix_from_covariance(covariance, f.sqrt_information)) return MSFL_BAD_ARG;
  *out = f;
  return MSFL_OK;
}

msfl_status msfl_graph_set_fixed(msfl_graph* g, int node, int flag) {
  msfl_status s = enter(g); if (s) return s;
  if (node < 0 || node >= g->n_nodes) return fail(g, MSFL_BAD_ARG, "msfl_graph_set_fixed: node index out of range");
  const unsigned char f = flag ? 1 : 0;
  if (g->fixed[node] != f) { g->fixed[node] = f; g->dirty = true; }
  return MSFL_OK;
}

msfl_status msfl_graph_set_poses(msfl_graph* g, int first, int n, const double* poses, msfl_mem mem) {
  msfl_status s = enter(g); if (s) return s;
  if (first < 0 || n < 0 || (long long)first + n > g->n_nodes || (n > 0 && !poses) || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE))
    return fail(g, MSFL_BAD_ARG, "msfl_graph_set_poses: range outside the nodes, null array or unknown memory kind");
  if (n == 0) return MSFL_OK;
  return graph_store_poses(g, "msfl_graph_set_poses", poses, first, n, mem);
}

msfl_status msfl_graph_get_poses(msfl_graph* g, int first, int n, double* out, msfl_mem mem) {
  msfl_status s = enter(g); if (s) return s;
  if (first < 0 || n < 0 || (long long)first + n > g->n_nodes || (n > 0 && !out) || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE))
    return fail(g, MSFL_BAD_ARG, "msfl_graph_get_poses: range outside the nodes, null array or unknown memory kind");
  if (n == 0) return MSFL_OK;
  HIPCHK(g, hipMemcpyAsync(out, g->x.as<double>() + (size_t)first * 7, (size_t)n * 7 * sizeof(double),
                           mem == MSFL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, g->stream));
  if (mem == MSFL_MEM_HOST) HIPCHK(g, hipStreamSynchronize(g->stream));
  return MSFL_OK;
}

msfl_status msfl_graph_cost(msfl_graph* g, double* cost) {
  msfl_status s = enter(g); if (s) return s;
  if (!cost) return fail(g, MSFL_BAD_ARG, "msfl_graph_cost: null result");
  *cost = 0.0;
  s = graph_prepare(g); if (s) return s;
  if (g->dev.n_factors == 0) return MSFL_OK;
  hipStream_t st = g->stream;
  double* d_out = g->dev.tr_cost + std::max(1, g->cfg.max_num_iterations);
  graph_enqueue_cost<false>(st, g->dev, g->dev.x, g->cfg.huber_delta, graph_losses(g));
  graph_launch(st, graph_cost_total_kernel, 1, kGraphVec, g->dev, d_out);
  HIPCHK(g, hipGetLastError());
  HIPCHK(g, hipMemcpyAsync(g->readback.p, d_out, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(g, hipStreamSynchronize(st));
  *cost = *g->readback.as<double>();
  return MSFL_OK;
}

msfl_status msfl_graph_factor_chi2(msfl_graph* g, int kind, int first, int n, double* out) {
  msfl_status s = enter(g); if (s) return s;
  int k0 = 0;
  if (!graph_factor_range(g, kind, first, n, &k0) || (n > 0 && !out))
    return fail(g, MSFL_BAD_ARG, "msfl_graph_factor_chi2: unknown kind, range outside the factors of that kind or null result");
  if (n == 0) return MSFL_OK;
  s = graph_prepare(g); if (s) return s;
  hipStream_t st = g->stream;
  HIPCHK(g, g->chi.reserve((size_t)n * sizeof(double)));
  graph_launch(st, graph_chi2_kernel, n, kGraphBlock, g->dev, k0, n, g->chi.as<double>());
  HIPCHK(g, hipGetLastError());
  HIPCHK(g, hipMemcpyAsync(out, g->chi.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(g, hipStreamSynchronize(st));
  return MSFL_OK;
}

msfl_status msfl_graph_factor_weights(msfl_graph* g, int kind, int first, int n, double* out) {
  msfl_status s = enter(g); if (s) return s;
  int k0 = 0;
  if (!graph_factor_range(g, kind, first, n, &k0) || (n > 0 && !out))
    return fail(g, MSFL_BAD_ARG, "msfl_graph_factor_weights: unknown kind, range outside the factors of that kind or null result");
  if (n == 0) return MSFL_OK;
  s = graph_prepare(g); if (s) return s;
  hipStream_t st = g->stream;
  HIPCHK(g, g->chi.reserve((size_t)n * sizeof(double)));
  if (g->has_losses) graph_launch(st, graph_weights_kernel<GraphLossDev>, n, kGraphBlock, g->dev, k0, n, g->chi.as<double>(), g->cfg.huber_delta, g->loss_dev);
  else graph_launch(st, graph_weights_kernel<>, n, kGraphBlock, g->dev, k0, n, g->chi.as<double>(), g->cfg.huber_delta);
  HIPCHK(g, hipGetLastError());
  HIPCHK(g, hipMemcpyAsync(out, g->chi.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(g, hipStreamSynchronize(st));
  return MSFL_OK;
}

msfl_status msfl_graph_set_losses(msfl_graph* g, int kind, int first, int n, const msfl_graph_loss* losses, int n_losses) {
  msfl_status s = enter(g); if (s) return s;
  int k0 = 0;
  if (!graph_factor_range(g, kind, first, n, &k0) || (n > 0 && !losses) || (n_losses != n && n_losses != 1))
    return fail(g, MSFL_BAD_ARG, "msfl_graph_set_losses: unknown factor kind, range outside the factors of that kind, null array or n_losses neither n nor 1; nothing set");
  for (int k = 0; k < (n > 0 ? n_losses : 0); k++)
    if (!graph_loss_ok(losses[k].kind, losses[k].a))
      return fail(g, MSFL_BAD_ARG, "msfl_graph_set_losses: an unknown loss kind, or a <= 0 or not finite on a kind that reads it; nothing set");
  if (n == 0) return MSFL_OK;
  const size_t held[4] = {g->edges.size(), g->fixes.size(), g->edges_info.size(), g->fixes_info.size()};
  HIPCHK(g, g->loss.reserve(std::max<size_t>(1, held[0] + held[1] + held[2] + held[3]) * (sizeof(double) + sizeof(int))));
  if (!g->has_losses) {
    for (int c = 0; c < 4; c++) g->losses[c].assign(held[c], msfl_graph_loss{MSFL_GRAPH_LOSS_DEFAULT, 0, 0.0});
    g->has_losses = true;
  }
  for (int k = 0; k < n; k++) {
    const msfl_graph_loss& l = losses[n_losses == 1 ? 0 : k];
    g->losses[kind][(size_t)first + k] = msfl_graph_loss{l.kind, 0, l.kind < MSFL_GRAPH_LOSS_HUBER ? 0.0 : l.a};
  }
  g->loss_dirty = true;
  return MSFL_OK;
}

msfl_status msfl_graph_get_losses(msfl_graph* g, int kind, int first, int n, msfl_graph_loss* out) {
  if (!g) return MSFL_BAD_ARG;
  int k0 = 0;
  if (!graph_factor_range(g, kind, first, n, &k0) || (n > 0 && !out))
    return fail(g, MSFL_BAD_ARG, "msfl_graph_get_losses: unknown factor kind, range outside the factors of that kind or null result");
  for (int k = 0; k < n; k++) out[k] = g->has_losses ? g->losses[kind][(size_t)first + k] : msfl_graph_loss{MSFL_GRAPH_LOSS_DEFAULT, 0, 0.0};
  return MSFL_OK;
}

msfl_status msfl_graph_optimize(msfl_graph* g, msfl_graph_summary* summary) {
  msfl_status s = enter(g); if (s) return s;
  if (!summary) return fail(g, MSFL_BAD_ARG, "msfl_graph_optimize: null summary");
  std::memset(summary, 0, sizeof(*summary));
  s = graph_prepare(g); if (s) return s;
  g->tr_accepted.clear(); g->tr_cost.clear();
  const GraphDev& d = g->dev;
  const GraphLevels& v = g->lv;
  summary->n_free = d.n_free; summary->n_long_edges = g->gs.n_long;
  if (d.n_free == 0 || d.n_factors == 0) { summary->termination = MSFL_GRAPH_EMPTY; return MSFL_OK; }
  hipStream_t st = g->stream;
  const GraphOpt o = graph_opt(g->cfg);
  GraphState init{};
  init.radius = o.radius0; init.decrease_factor = 2.0; init.step_successful = 1; init.first = 1;
  HIPCHK(g, g->pin.upload(g->state.p, &init, sizeof(init), st));
  HIPCHK(g, hipMemcpyAsync(d.cand, d.x, (size_t)d.n_nodes * 7 * sizeof(double), hipMemcpyDeviceToDevice, st));
  const int F = d.n_free, n_part = div_up(F, kGraphVec);
  const int direct = g->gs.n_long == 0;      // A == T: the preconditioner's solve is the step, one CG iteration
  const int cap = direct ? 1 : (g->cfg.max_cg_iterations > 0 ? g->cfg.max_cg_iterations : 16 * g->gs.n_long + 8);
  GraphState now{};
  for (int it = 0;; it++) {
    graph_launch(st, graph_commit_kernel, d.n_nodes * 7, kGraphVec, d);
    graph_enqueue_linearize(st, d, o.huber, graph_losses(g));
    graph_launch(st, graph_assemble_kernel, F, kGraphBlock, d);
    if (it == 0) graph_launch(st, graph_scale_kernel, F * 6, kGraphVec, d, o.jacobi);
    graph_launch(st, graph_tr_begin_kernel, 1, kGraphVec, d, o);
    if (it < o.max_iter) {
      graph_launch(st, graph_damp_kernel, F, kGraphVec, d, o);
      graph_enqueue_factor<false>(st, d, v, GraphMarg{}, 0.0);
      graph_enqueue_solve(st, d, v, 1, GraphSolveCols{});
      graph_launch(st, graph_dot_kernel, F, kGraphVec, d, n_part);
      for (int c = 0; c < cap; c++) {
        graph_launch(st, graph_matvec_kernel, F, kGraphVec, d, c, n_part, o.cg_tol, direct);
        graph_launch(st, graph_cg_update_kernel, F, kGraphVec, d, c, n_part);
        graph_enqueue_solve(st, d, v, 1, GraphSolveCols{});
        graph_launch(st, graph_dot_kernel, F, kGraphVec, d, n_part);
      }
      graph_launch(st, graph_cg_end_kernel, 1, kGraphVec, d, n_part, o.cg_tol, direct);
      graph_launch(st, graph_plus_kernel, F, kGraphVec, d);
      graph_enqueue_cost<true>(st, d, d.cand, o.huber, graph_losses(g));
      graph_launch(st, graph_tr_kernel, 1, kGraphVec, d, o);
    }
    HIPCHK(g, hipGetLastError());
    s = graph_read_state(g, &now); if (s) return s;          // the one read per LM iteration
    if (now.done) break;
    if (it >= o.max_iter) return fail(g, MSFL_HIP_ERROR, "msfl_graph_optimize: the device-side loop did not terminate");
  }
  summary->termination = now.termination; summary->iterations = now.iterations; summary->successful_steps = now.successful;
  summary->initial_cost = now.initial_cost; summary->final_cost = now.final_cost;
  summary->cg_iterations = now.cg_total; summary->cg_unconverged = now.cg_unconverged;
  const char* rb = g->readback.as<char>();
  const double* tc = reinterpret_cast<const double*>(rb + sizeof(GraphState));
  const int* ta = reinterpret_cast<const int*>(rb + sizeof(GraphState) + ((size_t)std::max(1, o.max_iter) + 1) * sizeof(double));
  g->tr_cost.assign(tc, tc + now.n_trace); g->tr_accepted.assign(ta, ta + now.n_trace);
  return MSFL_OK;
}

msfl_status msfl_graph_get_trace(msfl_graph* g, int* accepted, double* cost, int capacity, int* n_out) {
  if (!g) return MSFL_BAD_ARG;
  if (capacity < 0 || !n_out) return fail(g, MSFL_BAD_ARG, "msfl_graph_get_trace: negative capacity or null count");
  const int n = (int)g->tr_accepted.size();
  *n_out = n;
  for (int i = 0; i < std::min(n, capacity); i++) {
    if (accepted) accepted[i] = g->tr_accepted[i];
    if (cost) cost[i] = g->tr_cost[i];
  }
  return n > capacity ? fail(g, MSFL_CAPACITY, "msfl_graph_get_trace: the trace holds more iterations than `capacity`") : MSFL_OK;
}

// ---- marginals -----------------------------------------------------------------------------------------------------------------
void msfl_graph_marginals_default_options(msfl_graph_marginals_options* o) {
  if (!o) return;
  o->min_pivot_ratio = 1e-7; o->max_cg_iterations = 0; o->reserved = 0; o->scratch_bytes = 256ull << 20;
}

msfl_status msfl_graph_relative_covariance(const double* pose_a, const double* pose_b, const double* S_aa, const double* S_ab,
                                           const double* S_bb, double* out) {
  if (!pose_a || !pose_b || !S_aa || !S_ab || !S_bb || !out) return MSFL_BAD_ARG;
  return graph_relative_covariance(pose_a, pose_b, S_aa, S_ab, S_bb, out) ? MSFL_OK : MSFL_BAD_ARG;
}

msfl_status msfl_graph_marginals(msfl_graph* g, const int* pairs, int n_pairs, double* out, msfl_mem out_mem, msfl_graph_marginals_summary* summary) {
  return msfl_graph_marginals_with(g, pairs, n_pairs, out, out_mem, nullptr, summary);
}

msfl_status msfl_graph_marginals_with(msfl_graph* g, const int* pairs, int n_pairs, double* out, msfl_mem out_mem,
                                      const msfl_graph_marginals_options* options, msfl_graph_marginals_summary* summary) {
  msfl_status s = enter(g); if (s) return s;
  msfl_graph_marginals_summary local{};
  msfl_graph_marginals_summary* sm = summary ? summary : &local;
  msfl_graph_marginals_options opt;
  msfl_graph_marginals_default_options(&opt);
  if (options) opt = *options;
  if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !out)) || (out_mem != MSFL_MEM_HOST && out_mem != MSFL_MEM_DEVICE))
    return fail(g, MSFL_BAD_ARG, "msfl_graph_marginals: null array, negative count or unknown memory kind");
  if (!std::isfinite(opt.min_pivot_ratio) || opt.min_pivot_ratio < 0.0 || opt.max_cg_iterations < 0)
    return fail(g, MSFL_BAD_ARG, "msfl_graph_marginals: min_pivot_ratio not finite or negative, or a negative max_cg_iterations");
  for (int k = 0; k < 2 * n_pairs; k++)
    if (pairs[k] < 0 || pairs[k] >= g->n_nodes) return fail(g, MSFL_BAD_ARG, "msfl_graph_marginals: a node index out of range; nothing written");
  std::memset(sm, 0, sizeof(*sm));
  if (n_pairs == 0) return MSFL_OK;
  // the gauge the host can see: something has to tie the graph to the world, and free nodes need a factor
  const bool any_fixed = std::find(g->fixed.begin(), g->fixed.end(), (unsigned char)1) != g->fixed.end();
  const bool any_free = std::find(g->fixed.begin(), g->fixed.end(), (unsigned char)0) != g->fixed.end();
  const size_t n_fac = g->edges.size() + g->fixes.size() + g->edges_info.size() + g->fixes_info.size();
  if (!any_fixed && g->fixes.empty() && g->fixes_info.empty())
    return fail(g, MSFL_BAD_ARG, "msfl_graph_marginals: no fixed node and no fix: the graph is not anchored; nothing written");
  if (any_free && n_fac == 0) return fail(g, MSFL_BAD_ARG, "msfl_graph_marginals: free nodes but no factor; nothing written");
  s = graph_prepare(g); if (s) return s;
  hipStream_t st = g->stream;
  const GraphLevels& v = g->lv;
  const int F = g->dev.n_free;
  sm->n_pairs = n_pairs;
  const size_t out_bytes = (size_t)n_pairs * 36 * sizeof(double);
  if (F == 0) {                                            // every node fixed: zero variance everywhere
    sm->min_pivot_ratio = 1.0;
    if (out_mem == MSFL_MEM_HOST) std::memset(out, 0, out_bytes);
    else HIPCHK(g, hipMemsetAsync(out, 0, out_bytes, st));
    return MSFL_OK;
  }
  // the distinct free column nodes in the order they first appear, and per pair where its block lives
  std::vector<int> col_of((size_t)F, -1), ints;
  int n_cols = 0;
  for (int k = 0; k < n_pairs; k++) {
    const int fa = g->gs.free_of[pairs[2 * k]], fb = g->gs.free_of[pairs[2 * k + 1]];
    if (fa >= 0 && fb >= 0 && col_of[fb] < 0) { col_of[fb] = n_cols++; ints.push_back(fb); }
  }
  for (int k = 0; k < n_pairs; k++) ints.push_back(g->gs.free_of[pairs[2 * k]]);
  for (int k = 0; k < n_pairs; k++) {
    const int fa = g->gs.free_of[pairs[2 * k]], fb = g->gs.free_of[pairs[2 * k + 1]];
    ints.push_back(fa >= 0 && fb >= 0 ? col_of[fb] : -1);
  }
  const int n_part = div_up(F, kGraphBlock);
  const size_t upper = (size_t)v.off[v.count - 1] + 1 - (size_t)F;
  const size_t per_col = ((size_t)6 * F + 2 * upper) * 36 + (size_t)12 * n_part;             // doubles per column node
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_cols), (size_t)opt.scratch_bytes / (per_col * sizeof(double))));
  int n_piv = 0;
  for (int l = 0; l < v.tail; l++) n_piv += graph_invert_groups(v, l);
  const size_t state_bytes = sizeof(GraphState) + sizeof(GraphMargState) + (size_t)std::max(1, n_cols) * 6 * sizeof(GraphMargCol);
  HIPCHK(g, g->marg_work.reserve(((size_t)chunk * per_col + (size_t)std::max(1, n_piv)) * sizeof(double)));
  HIPCHK(g, g->marg_state.reserve(state_bytes));
  HIPCHK(g, g->marg_ints.reserve(ints.size() * sizeof(int)));
  HIPCHK(g, g->marg_read.reserve(std::max(sizeof(GraphMargState), (size_t)chunk * 6 * sizeof(GraphMargCol))));
  if (out_mem == MSFL_MEM_HOST) HIPCHK(g, g->marg_out.reserve(out_bytes));
  HIPCHK(g, g->pin.upload(g->marg_ints.p, ints.data(), ints.size() * sizeof(int), st));
  HIPCHK(g, hipMemsetAsync(g->marg_state.p, 0, sizeof(GraphState) + sizeof(GraphMargState), st));
  GraphDev d = g->dev;                                     // the reused kernels look at st->done, which the last optimize left at 1
  d.st = g->marg_state.as<GraphState>();
  GraphMarg M{};
  M.n_part = n_part;
  M.st = reinterpret_cast<GraphMargState*>(g->marg_state.as<char>() + sizeof(GraphState));
  GraphMargCol* cols = reinterpret_cast<GraphMargCol*>(g->marg_state.as<char>() + sizeof(GraphState) + sizeof(GraphMargState));
  const int* d_ints = g->marg_ints.as<int>();
  const int* d_pair_fa = d_ints + n_cols; const int* d_pair_col = d_pair_fa + n_pairs;
  double* d_out = out_mem == MSFL_MEM_HOST ? g->marg_out.as<double>() : out;
  auto carve_for = [&](int nc) {                           // the work area for a chunk of nc column nodes
    GraphCarve carve{g->marg_work.as<double>()};
    M.piv = carve((size_t)std::max(1, n_piv));
    const size_t blk = (size_t)nc * F * 36;
    M.X = carve(blk); M.R = carve(blk); M.Z = carve(blk); M.P[0] = carve(blk); M.P[1] = carve(blk); M.Q = carve(blk);
    M.rhs = carve((size_t)nc * upper * 36); M.sol = carve((size_t)nc * upper * 36);
    M.part = carve((size_t)12 * nc * n_part);
    M.n_cols = nc;
  };
  carve_for(0);
  // 1. linearise and assemble at the current poses, 2. the undamped level 0, 3. the factor half with the pivot test
  graph_enqueue_linearize(st, d, g->cfg.huber_delta, graph_losses(g));
  graph_launch(st, graph_assemble_kernel, F, kGraphBlock, d);
  graph_launch(st, graph_marg_setup_kernel, F, kGraphVec, d);
  graph_enqueue_factor<true>(st, d, v, M, opt.min_pivot_ratio);
  HIPCHK(g, hipGetLastError());
  HIPCHK(g, hipMemcpyAsync(g->marg_read.p, M.st, sizeof(GraphMargState), hipMemcpyDeviceToHost, st));
  HIPCHK(g, hipStreamSynchronize(st));
  const GraphMargState ms = *g->marg_read.as<GraphMargState>();
  sm->min_pivot_ratio = ms.min_pivot; sm->singular = ms.singular;
  const int gather_items = n_pairs * 36;
  if (ms.singular) {
    graph_launch(st, graph_marg_gather_kernel, gather_items, kGraphVec, d, M, d_pair_fa, d_pair_col, n_pairs, 0, 1, d_out);
  } else {
    const int direct = g->gs.n_long == 0;
    const int cap = opt.max_cg_iterations > 0 ? opt.max_cg_iterations : 16 * g->gs.n_long + 8;
    const double tol = g->cfg.cg_tolerance;
    if (n_cols == 0) graph_launch(st, graph_marg_gather_kernel, gather_items, kGraphVec, d, M, d_pair_fa, d_pair_col, n_pairs, 0, 0, d_out);
    for (int first = 0; first < n_cols; first += chunk) {
      carve_for(std::min(chunk, n_cols - first));
      M.col_free = d_ints + first; M.col = cols + (size_t)first * 6;
      graph_launch_y(st, graph_marg_init_kernel, F * 36, kGraphVec, M.n_cols, d, M);
      if (direct) {
        graph_enqueue_solve(st, d, v, M.n_cols, GraphMargCols{M, M.R, M.X});
      } else {
        graph_enqueue_solve(st, d, v, M.n_cols, GraphMargCols{M, M.R, M.Z});
        graph_launch_y(st, graph_marg_dot_kernel, F, kGraphBlock, M.n_cols, d, M);
        for (int it = 0; it < cap;) {                      // slices of at most 32 iterations, one small read between them
          for (const int end = std::min(cap, it + 32); it < end; it++) {
            graph_launch_y(st, graph_marg_matvec_kernel, F, kGraphBlock, M.n_cols, d, M, it, tol);
            graph_launch_y(st, graph_marg_update_kernel, F, kGraphBlock, M.n_cols, d, M, it);
            graph_enqueue_solve(st, d, v, M.n_cols, GraphMargCols{M, M.R, M.Z});
            graph_launch_y(st, graph_marg_dot_kernel, F, kGraphBlock, M.n_cols, d, M);
          }
          graph_launch(st, graph_marg_check_kernel, M.n_cols * kGraphBlock, kGraphBlock, M, it, tol);
          HIPCHK(g, hipGetLastError());
          HIPCHK(g, hipMemcpyAsync(g->marg_read.p, M.col, (size_t)M.n_cols * 6 * sizeof(GraphMargCol), hipMemcpyDeviceToHost, st));
          HIPCHK(g, hipStreamSynchronize(st));
          const GraphMargCol* hc = g->marg_read.as<GraphMargCol>();
          int running = 0;
          for (int k = 0; k < M.n_cols * 6; k++) running += !hc[k].done;
          if (running && it < cap) continue;
          for (int k = 0; k < M.n_cols * 6; k++) sm->cg_iterations = std::max(sm->cg_iterations, hc[k].it);
          sm->cg_unconverged += running;
          break;
        }
      }
      graph_launch(st, graph_marg_gather_kernel, gather_items, kGraphVec, d, M, d_pair_fa, d_pair_col, n_pairs, first, 0, d_out);
    }
  }
  sm->n_columns = ms.singular ? 0 : 6 * n_cols;
  HIPCHK(g, hipGetLastError());
  if (out_mem == MSFL_MEM_HOST) {
    HIPCHK(g, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(g, hipStreamSynchronize(st));
  }
  return MSFL_OK;
}

}  // extern "C"
