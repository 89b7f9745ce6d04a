// abi_measure.inc — C-ABI entry points: finite-shot measurement (measure_host.inc).  Included by ovqe_sv.hip inside extern "C".

static int measure_args(ovqe_handle h, const char *who, uint64_t xbasis, uint64_t ybasis, int64_t n_shots) {
    int rc = measure_applicable(h, who);
    if (rc) return rc;
    if (n_shots < 0 || n_shots > ((int64_t)1 << 31)) return fail(h, OVQE_ERR_INVALID, std::string(who) + ": n_shots must lie in [0, 2^31]");
    if (!measure::basis_ok(h->n_local, xbasis, ybasis))
        return fail(h, OVQE_ERR_INVALID, std::string(who) + ": xbasis and ybasis must be disjoint masks of index bits inside the register");
    return OVQE_OK;
}

int ovqe_sample(ovqe_handle h, int64_t n_shots, uint64_t seed, uint64_t stream, uint64_t first_shot, uint64_t *indices) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    int rc = measure_args(h, "ovqe_sample", 0, 0, n_shots);
    if (rc) return rc;
    if (n_shots > 0 && !indices) return fail(h, OVQE_ERR_INVALID, "ovqe_sample: indices is NULL");
    return run_measure(h, 0, 0, n_shots, seed, stream, first_shot, 0, nullptr, nullptr, nullptr, nullptr, indices, "ovqe_sample");
} OVQE_CATCH(h)

int ovqe_measure_paulis(ovqe_handle h, uint64_t xbasis, uint64_t ybasis, int64_t n_shots, uint64_t seed, uint64_t stream, uint64_t first_shot,
                        int64_t T, const uint64_t *mask, const double *coeff, int64_t *term_sums, double *value_sums, uint64_t *indices) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    int rc = measure_args(h, "ovqe_measure_paulis", xbasis, ybasis, n_shots);
    if (rc) return rc;
    if (T < 0 || T > 0x7fffffff) return fail(h, OVQE_ERR_INVALID, "ovqe_measure_paulis: T out of range");
    if (T > 0 && (!mask || !coeff || !term_sums)) return fail(h, OVQE_ERR_INVALID, "ovqe_measure_paulis: mask, coeff or term_sums is NULL");
    if (!value_sums) return fail(h, OVQE_ERR_INVALID, "ovqe_measure_paulis: value_sums is NULL");
    return run_measure(h, xbasis, ybasis, n_shots, seed, stream, first_shot, T, mask, coeff, term_sums, value_sums, indices, "ovqe_measure_paulis");
} OVQE_CATCH(h)

int ovqe_measure_groups(ovqe_handle h, int64_t capacity, int32_t *group_of_term, uint64_t *xbasis, uint64_t *ybasis, int64_t *n_groups) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (!n_groups || capacity < 0 || (capacity > 0 && (!group_of_term || !xbasis || !ybasis)))
        return fail(h, OVQE_ERR_INVALID, "ovqe_measure_groups: NULL argument");
    int rc = measure_applicable(h, "ovqe_measure_groups");
    if (rc) return rc;
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "ovqe_measure_groups: no Hamiltonian set (ovqe_set_hamiltonian)");
    MeasureDev &M = measure_dev(h);
    if ((rc = measure_plan(h, M))) return rc;
    const int64_t T = (int64_t)M.plan.group_of_term.size(), G = M.plan.groups();
    for (int64_t t = 0; t < T && t < capacity; ++t) group_of_term[t] = M.plan.group_of_term[t];
    for (int64_t g = 0; g < G && g < capacity; ++g) {
        xbasis[g] = M.plan.xbasis[g];
        ybasis[g] = M.plan.ybasis[g];
    }
    *n_groups = G;
    return OVQE_OK;
} OVQE_CATCH(h)

int ovqe_energy_sampled(ovqe_handle h, const double *theta, int32_t K, int64_t n_shots, uint64_t seed, double *energy, double *std_error) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (!energy || !std_error) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_sampled: energy or std_error is NULL");
    int rc = measure_args(h, "ovqe_energy_sampled", 0, 0, n_shots);
    if (rc) return rc;
    if (n_shots < 2) return fail(h, OVQE_ERR_INVALID, "ovqe_energy_sampled: n_shots must be at least 2 (the sample variance divides by n_shots - 1)");
    if (!h->ham.set) return fail(h, OVQE_ERR_STATE, "ovqe_energy_sampled: no Hamiltonian set (ovqe_set_hamiltonian)");
    if ((rc = ovqe_prepare_state(h, theta, K))) return rc;
    return run_energy_sampled(h, n_shots, seed, energy, std_error);
} OVQE_CATCH(h)

int ovqe_measure_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    if (!h || !info || count < 0) return OVQE_ERR_INVALID;
    for (int i = 0; i < count && i < 9; ++i) info[i] = h->measure ? h->measure->info[i] : 0;
    return OVQE_OK;
} OVQE_CATCH(h)
