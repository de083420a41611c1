// mgx_world_mirror.inc — SoA helpers, blob <-> host mirror, pull (device -> host mirror).
// Part of ONE translation unit: included by mgx_world.hip (which says in which order, and why one unit).
// ---- SoA helpers --------------------------------------------------------------------------------
template <class T>
static void scatter(std::vector<T> &dst, size_t stride, size_t item, const T *src, int comps) {
    for (int c = 0; c < comps; c++) dst[(size_t)c * stride + item] = src[c];
}
template <class T>
static void gather(const std::vector<T> &src, size_t stride, size_t item, T *dst, int comps) {
    for (int c = 0; c < comps; c++) dst[c] = src[(size_t)c * stride + item];
}

// J^T Q J of a dynamic factor in the reference's evaluation order (dynamic.rs:22-52,
// factor/mod.rs:391-394), compacted to the 4x4 M with lam_p = M (x) I2.
static void dynamic_potential(double dt, double sigma, double *M /*16*/) {
    const double qc = 1.0 / (sigma * sigma);
    const double q11 = 12.0 * (1.0 / (dt * dt * dt)) * qc, q12 = -6.0 * (1.0 / (dt * dt)) * qc, q22 = (4.0 / dt) * qc;
    double Q[16] = {0}, J[32] = {0};
    for (int a = 0; a < 2; a++) {
        Q[a * 4 + a] = q11;
        Q[a * 4 + a + 2] = q12;
        Q[(a + 2) * 4 + a] = q12;
        Q[(a + 2) * 4 + a + 2] = q22;
        J[a * 8 + a] = 1.0;
        J[a * 8 + a + 2] = dt;
        J[a * 8 + a + 4] = -1.0;
        J[(a + 2) * 8 + a + 2] = 1.0;
        J[(a + 2) * 8 + a + 6] = -1.0;
    }
    double JtQ[32], L[64];
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += J[k * 8 + i] * Q[k * 4 + j];
            JtQ[i * 4 + j] = s;
        }
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += JtQ[i * 4 + k] * J[k * 8 + j];
            L[i * 8 + j] = s;
        }
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) M[a * 4 + b] = L[(2 * a) * 8 + (2 * b)];
}

// ---- blob <-> host mirror -----------------------------------------------------------------------------
// rows of a robot's blob are component-major ([c][K] / [c][E+1]); the host mirror is item-major
static void blob_pack(const Robot &rb, double *b) {
    const int K = rb.K, E = 4 * K - 6, E1 = E + 1;
    const BlobLayout L(K);
    for (int i = 0; i < K; i++) {
        for (int c = 0; c < 4; c++) {
            b[L.prior() + c * K + i] = rb.prior_eta[4 * i + c];
            b[L.bel() + c * K + i] = rb.bel_eta[4 * i + c];
            b[L.mu() + c * K + i] = rb.bel_mu[4 * i + c];
        }
        for (int c = 0; c < 16; c++) {
            b[L.prior() + (4 + c) * K + i] = rb.prior_lam[16 * i + c];
            b[L.bel() + (4 + c) * K + i] = rb.bel_lam[16 * i + c];
            b[L.cov() + c * K + i] = rb.bel_cov[16 * i + c];
        }
    }
    for (int c = 0; c < 20; c++) b[L.fv() + c * E1 + E] = 0.0;  // the all-zero column
    if (!rb.ghost)
        for (int e = 0; e < E; e++) {
            for (int c = 0; c < 4; c++) b[L.fv() + c * E1 + e] = rb.fv_eta[4 * e + c];
            for (int c = 0; c < 16; c++) b[L.fv() + (4 + c) * E1 + e] = rb.fv_lam[16 * e + c];
        }
    int32_t *valid = reinterpret_cast<int32_t *>(b + L.valid());
    for (int i = 0; i < K; i++) valid[i] = rb.valid[i];
}
static void blob_unpack(Robot &rb, const double *b) {
    const int K = rb.K, E = 4 * K - 6, E1 = E + 1;
    const BlobLayout L(K);
    for (int i = 0; i < K; i++) {
        for (int c = 0; c < 4; c++) {
            rb.prior_eta[4 * i + c] = b[L.prior() + c * K + i];
            rb.bel_eta[4 * i + c] = b[L.bel() + c * K + i];
            rb.bel_mu[4 * i + c] = b[L.mu() + c * K + i];
        }
        for (int c = 0; c < 16; c++) {
            rb.prior_lam[16 * i + c] = b[L.prior() + (4 + c) * K + i];
            rb.bel_lam[16 * i + c] = b[L.bel() + (4 + c) * K + i];
            rb.bel_cov[16 * i + c] = b[L.cov() + c * K + i];
        }
    }
    if (!rb.ghost)
        for (int e = 0; e < E; e++) {
            for (int c = 0; c < 4; c++) rb.fv_eta[4 * e + c] = b[L.fv() + c * E1 + e];
            for (int c = 0; c < 16; c++) rb.fv_lam[16 * e + c] = b[L.fv() + (4 + c) * E1 + e];
        }
    const int32_t *valid = reinterpret_cast<const int32_t *>(b + L.valid());
    for (int i = 0; i < K; i++) rb.valid[i] = valid[i];
}

// ---- pull: device -> host mirror ----------------------------------------------------------------
static int pull(mgx_world *w) {
    if (!w->dev_valid) return MGX_OK;
    MGX_CONFIRM(w);
    w->n_pulls++;
    const int K = w->K;
    const size_t NT = (size_t)w->d.NT, NI = (size_t)w->d.NI, BS = (size_t)w->d.BS;
    std::vector<double> bl, sn, tlv, ife, ifl, ibm;
    std::vector<int32_t> trc, itf;
    std::vector<uint32_t> ep;
    std::vector<float> tlp;
    hipStream_t s = w->stream;
    HIP_TRY(w->blob.download(bl, s));
    HIP_TRY((w->d.cur ? w->snap1 : w->snap0).download(sn, s));
    HIP_TRY((w->d.cur ? w->epoch1 : w->epoch0).download(ep, s));
    HIP_TRY(w->trk_record.download(trc, s));
    HIP_TRY(w->trk_last_pos.download(tlp, s));
    HIP_TRY(w->trk_last_val.download(tlv, s));
    HIP_TRY(w->iter_factor.download(itf, s));
    HIP_TRY(w->ir_fv_eta.download(ife, s));
    HIP_TRY(w->ir_fv_lam.download(ifl, s));
    HIP_TRY(w->ir_bmu.download(ibm, s));
    std::vector<IrEdgeRec> irc;
    HIP_TRY(w->ir_rec.download(irc, s));
    std::vector<double> fzd;
    std::vector<uint8_t> fzf, thw;
    if (w->frozen_live) {
        HIP_TRY(w->frozen_buf.download(fzd, s));
        HIP_TRY(w->frozen_flag_buf.download(fzf, s));
        HIP_TRY(w->thaw_buf.download(thw, s));
    }
    std::vector<double> ifs;
    std::vector<uint32_t> ife_, ite;
    if (w->ir_frozen_live) {
        HIP_TRY(w->ir_frozen_snap_buf.download(ifs, s));
        HIP_TRY(w->ir_frozen_epoch_buf.download(ife_, s));
        if (w->ir_thaw_active) HIP_TRY(w->ir_thaw_epoch_buf.download(ite, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t dr = 0; dr < w->robot_of.size(); dr++) {
        Robot &rb = w->robots[(size_t)w->robot_of[dr]];
        blob_unpack(rb, &bl[dr * BS]);
        if (w->ir_frozen_live) {
            rb.ir_frozen_snap.assign(ifs.begin() + (long)(dr * K * 24), ifs.begin() + (long)((dr + 1) * K * 24));
            rb.ir_frozen_epoch.assign(ife_.begin() + (long)(dr * K), ife_.begin() + (long)((dr + 1) * K));
            if (w->ir_thaw_active) rb.ir_thaw_epoch.assign(ite.begin() + (long)(dr * K), ite.begin() + (long)((dr + 1) * K));
        }
        for (int i = 0; i < K; i++) {
            const size_t v = dr * K + i;
            memcpy(&rb.snap[24 * i], &sn[v * 24], 24 * sizeof(double));
            rb.epoch[i] = ep[v];
        }
        if (rb.ghost) continue;
        for (int j = 0; j < K - 2; j++) {
            const size_t t = dr * (K - 2) + j;
            rb.trk_record[j] = trc[t];
            rb.trk_last_pos[2 * j] = tlp[t];
            rb.trk_last_pos[2 * j + 1] = tlp[NT + t];
            rb.trk_last_val[j] = tlv[t];
        }
        rb.iter_factor = itf[dr];
        if (w->frozen_live) {
            const size_t FZ = (size_t)frozen_words(K), E = (size_t)(4 * K - 6);
            rb.frozen.assign(fzd.begin() + (long)(dr * FZ), fzd.begin() + (long)((dr + 1) * FZ));
            rb.frozen_flag.assign(fzf.begin() + (long)(dr * E), fzf.begin() + (long)((dr + 1) * E));
            rb.thaw = thw[dr];
        }
    }
    for (size_t ci = 0; ci < w->conns.size(); ci++) {
        IrConn &c = w->conns[ci];
        const int32_t dev_slot = dev_slot_of(w, ci);
        for (size_t j = 0; j < c.edges.size(); j++) {
            if (dev_slot < 0) continue;  // created since the tables were built: nothing on the device yet
            const size_t e = edge_index(w->dev_in_ptr, w->K, w->dev_of[(size_t)c.other], (int)j, dev_slot);
            IrEdge &ed = c.edges[j];
            gather(ife, NI, e, ed.fv_eta, 4);
            gather(ifl, NI, e, ed.fv_lam, 16);
            gather(ibm, NI, e, ed.bmu, 4);
            ed.created = irc[e].created;  // edges born in an in-place rebuild got theirs on the device
            // compact messages: only eta[0..2) and lam[0..2)x[0..2) are kept on the device
            ed.fv_eta[2] = ed.fv_eta[3] = 0.0;
            for (int q = 0; q < 16; q++)
                if ((q >> 2) >= 2 || (q & 3) >= 2) ed.fv_lam[q] = 0.0;
        }
    }
    return MGX_OK;
}
