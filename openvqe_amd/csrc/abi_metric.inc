// abi_metric.inc — C-ABI entry points: Fubini-Study metric of the ansatz state (metric_host.inc).
// Included by ovqe_sv.hip inside extern "C".

int ovqe_metric_tensor(ovqe_handle h, const double *theta, int32_t K, double *metric) try {
    OVQE_ENTER(h);
    if (!h) return OVQE_ERR_INVALID;
    if (!metric) return fail(h, OVQE_ERR_INVALID, "ovqe_metric_tensor: metric is NULL");
    if (h->n_global > 0) return fail(h, OVQE_ERR_STATE, "ovqe_metric_tensor: not available on a shard of a partitioned register");
    if (h->opt_real_state) return fail(h, OVQE_ERR_STATE, "ovqe_metric_tensor: not available under option real_state (the buffer holds 8-byte amplitudes)");
    if (!h->prog_set) return fail(h, OVQE_ERR_STATE, "ovqe_metric_tensor: no program set (ovqe_set_program / ovqe_set_gate_program)");
    if (K != h->K) return fail(h, OVQE_ERR_INVALID, "ovqe_metric_tensor: K = " + std::to_string(K) + ", the program has " + std::to_string(h->K) + " parameters");
    if (K > 0 && !theta) return fail(h, OVQE_ERR_INVALID, "ovqe_metric_tensor: theta is NULL");
    return run_metric(h, theta, metric);
} OVQE_CATCH(h)

int ovqe_metric_info(ovqe_handle h, int64_t *info, int count) try {
    OVQE_ENTER(h);
    if (!h || !info || count < 0) return OVQE_ERR_INVALID;
    for (int i = 0; i < count && i < 11; ++i) info[i] = h->metric ? h->metric->info[i] : 0;
    return OVQE_OK;
} OVQE_CATCH(h)
