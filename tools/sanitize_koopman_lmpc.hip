// sanitize_koopman_lmpc.hip -- a stand-alone program (its own main, no interpreter) that drives the host side of edmdc_lmpc_step /
// edmdc_lmpc_step_dev under AddressSanitizer and UndefinedBehaviourSanitizer: every refusal of the header, the empty call, and a
// well-formed call on a host without a device (which must come back with an error code, not a crash).  It includes capi.hip so that
// it can make a brov_ctx without a device (brov_create needs one); nothing here touches a GPU.
//
// Build and run (CPU only): tools/sanitize_koopman_lmpc.sh.
// Prints one line per group and "clean: N checks"; exit status 0 only if every check held and no sanitizer report was raised.
#include "../bluerov2_dynamics_amd/csrc/capi.hip"

#include <limits>

namespace {

int checks = 0, failures = 0;
constexpr int NB = 3, HS = 7, HOLD = 3, MS = 3, N = 12, R = 8, KC = 4, REF_TOTAL = 12, ROW0 = 2, NV = MS * R;
constexpr double PAT = -7.25;

struct Call {
    brov_lmpc cfg;
    int n = N, r = R, k = KC;
    double gamma = 1.0, dt = 0.05;
    int64_t nb = NB, H = HS, ref_total = REF_TOTAL, row0 = ROW0;
    bool null_cfg = false, null_x = false, null_ref = false, null_U = false, null_A = false, null_B = false, null_P = false, null_Gc = false,
         null_C = false, null_W = false;
    Call() {
        for (int i = 0; i < 13; ++i) { cfg.q[i] = 1.0; cfg.qf[i] = 2.0; }
        for (int i = 0; i < 8; ++i) { cfg.r[i] = 0.1; cfg.u_min[i] = -0.7; cfg.u_max[i] = 0.7; }
        cfg.rho = 1.5; cfg.tol = 1e-6; cfg.hold = HOLD; cfg.iters = 20;
    }
};

// exactly the sizes the header states, so that a read or write past them is a sanitizer report
struct Buffers {
    std::vector<double> C, A, B, P, Gc, W, x, ref, U, y, ua, pred, info;
    Buffers() : C(KC * N, 0.1), A((N + KC) * (N + KC), 0.0), B((N + KC) * R, 0.01), P((HS + 1) * N * (N + KC), 0.0), Gc((HS + 1) * MS * N * R, 0.0),
                W(NV * NV, 0.0), x(NB * N, 0.2), ref(NB * REF_TOTAL * N, 0.1), U(NB * NV, 0.05), y(NB * NV, 0.01), ua(NB * HOLD * R, PAT),
                pred(NB * (HS + 1) * N, PAT), info(NB * 6, PAT) {}
    bool untouched() const {
        for (const auto* v : {&ua, &pred, &info})
            for (double e : *v) if (e != PAT) return false;
        for (double e : U) if (e != 0.05) return false;
        for (double e : y) if (e != 0.01) return false;
        return true;
    }
};

int run(brov_ctx* c, const Call& a, Buffers& b, bool dev) {
    auto fn = dev ? edmdc_lmpc_step_dev : edmdc_lmpc_step;
    return fn(c, a.n, a.r, a.k, a.gamma, a.null_C ? nullptr : b.C.data(), a.null_A ? nullptr : b.A.data(), a.null_B ? nullptr : b.B.data(),
              a.null_P ? nullptr : b.P.data(), a.null_Gc ? nullptr : b.Gc.data(), a.null_W ? nullptr : b.W.data(), a.nb, a.null_cfg ? nullptr : &a.cfg,
              a.H, a.dt, a.null_x ? nullptr : b.x.data(), a.null_ref ? nullptr : b.ref.data(), a.ref_total, a.row0,
              a.null_U ? nullptr : b.U.data(), b.y.data(), 1, b.ua.data(), b.pred.data(), b.info.data());
}

void refused(brov_ctx* c, const char* want, const Call& a) {
    for (int dev = 0; dev < 2; ++dev) {
        Buffers b;
        c->err.clear();
        const int rc = run(c, a, b, dev != 0);
        ++checks;
        if (rc != BROV_ERR_ARG || c->err.find(want) == std::string::npos || c->err.rfind("edmdc_lmpc_step: ", 0) != 0 || !b.untouched()) {
            ++failures;
            std::printf("FAILED: want \"%s\", got rc %d, \"%s\", outputs %s\n", want, rc, c->err.c_str(), b.untouched() ? "untouched" : "WRITTEN");
        }
    }
}

}  // namespace

int main() {
    brov_ctx ctx;                       // no device behind it: everything below is decided on the host
    brov_ctx* c = &ctx;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    { Call a; a.H = 0; refused(c, "H must be >= 1", a); }
    { Call a; a.H = ((int64_t)1 << 31) + 1; a.ref_total = 1; a.row0 = 0; refused(c, "H must be <= 2^31", a); }
    { Call a; a.row0 = REF_TOTAL - HS; refused(c, "reference window", a); }
    { Call a; a.row0 = -1; refused(c, "reference window", a); }
    { Call a; a.ref_total = 1; a.row0 = 1; refused(c, "reference window", a); }
    { Call a; a.ref_total = 0; a.row0 = 0; refused(c, "reference window", a); }
    { Call a; a.nb = 65536; refused(c, "B must be <= 65535", a); }
    { Call a; a.nb = -1; refused(c, "negative size", a); }
    for (double dt : {0.0, -0.02, inf, nan}) { Call a; a.dt = dt; refused(c, "dt must be finite and > 0", a); }
    { Call a; a.null_cfg = true; refused(c, "NULL input", a); }
    { Call a; a.null_x = true; refused(c, "NULL input", a); }
    { Call a; a.null_ref = true; refused(c, "NULL input", a); }
    { Call a; a.null_U = true; refused(c, "NULL input", a); }
    for (int n : {0, 11, 14, -12}) { Call a; a.n = n; refused(c, "n must be 12 (Euler angles) or 13 (quaternion)", a); }
    for (int r : {0, 7, 9, -8}) { Call a; a.r = r; refused(c, "r must be 6 or 8", a); }
    { Call a; a.k = -1; refused(c, "k must be >= 0", a); }
    { Call a; a.k = 1025; refused(c, "k must be <= 1024", a); }
    { Call a; a.null_A = true; refused(c, "NULL A, B, P or Gc", a); }
    { Call a; a.null_B = true; refused(c, "NULL A, B, P or Gc", a); }
    { Call a; a.null_P = true; refused(c, "NULL A, B, P or Gc", a); }
    { Call a; a.null_Gc = true; refused(c, "NULL A, B, P or Gc", a); }
    { Call a; a.null_C = true; refused(c, "NULL C with k > 0", a); }
    { Call a; a.gamma = nan; refused(c, "NaN gamma", a); }
    { Call a; a.cfg.hold = 1; a.H = 40; a.ref_total = 1; a.row0 = 0; refused(c, "M nu = 320 must be <= 312", a); }
    { Call a; a.r = 6; a.cfg.hold = 1; a.H = 53; a.ref_total = 1; a.row0 = 0; refused(c, "M nu = 318 must be <= 312", a); }
    std::printf("the rules shared with edmdc_mppi_step: %d checks, %d failed\n", checks, failures);
    { Call a; a.null_W = true; refused(c, "NULL W", a); }
    { Call a; a.cfg.hold = 0; refused(c, "hold must be >= 1", a); }
    { Call a; a.cfg.hold = -3; refused(c, "hold must be >= 1", a); }
    { Call a; a.cfg.iters = -1; refused(c, "iters must be 0 .. 1 000 000", a); }
    { Call a; a.cfg.iters = 1000001; refused(c, "iters must be 0 .. 1 000 000", a); }
    for (double rho : {0.0, -1.0, inf}) { Call a; a.cfg.rho = rho; refused(c, "rho must be finite and > 0", a); }
    { Call a; a.cfg.rho = nan; refused(c, "NaN in the record", a); }
    { Call a; a.cfg.tol = -1e-9; refused(c, "tol must be >= 0", a); }
    { Call a; a.cfg.tol = nan; refused(c, "NaN in the record", a); }
    { Call a; a.cfg.q[3] = -1.0; refused(c, "q and qf must be >= 0", a); }
    { Call a; a.cfg.qf[11] = -1.0; refused(c, "q and qf must be >= 0", a); }
    { Call a; a.cfg.r[0] = -0.5; refused(c, "r must be >= 0", a); }
    { Call a; a.cfg.u_min[7] = 2.0; refused(c, "u_min must be <= u_max", a); }
    { Call a; a.cfg.qf[2] = nan; refused(c, "NaN in the record", a); }
    { Call a; a.cfg.u_max[5] = nan; refused(c, "NaN in the record", a); }
    std::printf("the rules of the record and W: %d checks, %d failed\n", checks, failures);
    for (int dev = 0; dev < 2; ++dev) { // nb = 0: BROV_OK and nothing touched, whatever else is passed; a NULL context: BROV_ERR_ARG
        Buffers b;
        Call a;
        a.nb = 0;
        ++checks;
        if (run(c, a, b, dev != 0) != BROV_OK || !b.untouched()) { ++failures; std::printf("FAILED: nb = 0\n"); }
        Call g;
        ++checks;
        if (run(nullptr, g, b, dev != 0) != BROV_ERR_ARG || !b.untouched()) { ++failures; std::printf("FAILED: NULL context\n"); }
    }
    {                                   // entry 12 of q and the channels >= nu are ignored: a negative weight there is no refusal; and a
        Buffers b;                      // well-formed call (k = 0 without centres is one) passes every check, then has no device to run on
        Call a;
        a.k = 0;
        a.null_C = true;
        a.r = 6;
        a.cfg.q[12] = -1.0;
        a.cfg.r[7] = -1.0;
        a.cfg.u_min[6] = 3.0;
        b.A.assign(N * N, 0.0);
        const int rc = run(c, a, b, false);
        ++checks;
        if (rc == BROV_OK || rc == BROV_ERR_ARG) { ++failures; std::printf("FAILED: a call without a device returned %d (%s)\n", rc, c->err.c_str()); }
        else std::printf("a well-formed call without a device: rc %d, \"%s\"\n", rc, c->err.c_str());
    }
    if (failures) { std::printf("%d of %d checks FAILED\n", failures, checks); return 1; }
    std::printf("clean: %d checks\n", checks);
    return 0;
}
