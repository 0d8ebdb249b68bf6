// BlockOrthHost.hpp -- the host arithmetic of the coordinate back end's block orthogonalisation (SubspaceWrappers.hpp: block CGS2 against
// the basis, CholQR2 inside the block, the overlapped form's prediction and read-back), on small column-major matrices.  Nothing here
// knows of SubspaceBasis, of a context or of the device, so all of it runs and is tested without a GPU (tests/cpp/block_orth_host.cpp).
//
// Results are part of the solver's bit-for-bit reproducibility: every sum below keeps its loop order and every expression its shape
// (the host code is compiled with contraction inside one expression).
#ifndef RAILS_BLOCKORTHHOST_HPP
#define RAILS_BLOCKORTHHOST_HPP

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "rails_hip.h"

namespace rails
{

// coefficient block: column-major, ld rows of capacity (rows past the basis dimension are zero), ncap columns
struct CoefStore {
    std::vector<double> c;
    int ld = 0, ncap = 0;
    bool in_basis = true; // false: a plain small replicated matrix with ld rows (B'W and friends)
    CoefStore(int ld_, int ncap_, bool in_basis_) : c((size_t)std::max(ld_, 1) * std::max(ncap_, 1), 0.0), ld(ld_), ncap(std::max(ncap_, 1)), in_basis(in_basis_) {}
    double *col(int j) { return c.data() + (size_t)j * ld; }
    const double *col(int j) const { return c.data() + (size_t)j * ld; }
    // column j holds something in its rows [from, dim)
    bool in_use(int j, int dim, int from = 0) const
    {
        for (const double *x = col(j) + from; x < col(j) + dim; ++x)
            if (*x != 0.0) return true;
        return false;
    }
};

namespace block_orth
{

// ---- the thresholds ------------------------------------------------------------------------------------------------------------------
// Fractions are of a column's squared length before any projection; diagonals are those of the Cholesky factor of the block's Gram matrix
// scaled to a unit diagonal.
constexpr double reorth_survival = 0.5;       // DGKS: a column that keeps no more than this after one projection is projected again
constexpr double drop_fraction = 1e-26;       // less than this left after the projections: the column lies in span(P)
constexpr double delicate_fraction = 1e-8;    // less than this left: direction or rounding error?  Normalise, project once more ...
constexpr double delicate_keep = 0.25;        // ... and keep what retains more than this of its unit squared length
constexpr double dependent_diag = 1e-6;       // a diagonal not above this: the block's columns depend on each other, taken one by one
constexpr double reproject_diag = 1e-2;       // a diagonal below this: the block is projected once more after its CholQR
constexpr double single_drop_fraction = 1e-24; // the drop rule of the column-by-column form
// The overlapped form takes a block on only if, by Pythagoras (relative error eps / survival <= 1e-12), every column keeps at least
// overlap_min_survival of its squared length, more than delicate_fraction is left of each, and the predicted factor's diagonal is above
// reproject_diag.  Its read-back asks for readback_min_fraction and readback_min_diag and for the predicted factor to match the real one
// to readback_max_off: four to ten orders of magnitude below the start conditions.  A block that misses those means the device did not
// meet the block the host was promised (a faulted kernel, non-finite data): by then the host has used the predicted coordinates in a
// projected solve and a Lanczos run, and the block itself has been overwritten in place -- there is nothing sound to fall back to, so the
// failure is latched (SubspaceBasis::failed), reported on stderr, and ends the run at the next trip (Solver::set_failure_check);
// rails_solver_solve returns RAILS_EHIP.  Blocks that need the careful treatment (nearly dependent columns, directions already in
// span(P)) never get there: they fail the start conditions and take the synchronous path.
constexpr double overlap_min_survival = 1e-4; // below: rounding in the Pythagorean Gram matrix (eps / survival) is no longer negligible
constexpr double readback_min_fraction = 1e-8, readback_min_diag = 1e-6, readback_max_off = 1e-4;

inline double dot(const double *x, const double *y, int n)
{
    double s = 0.0; // (one running sum, in order: the results are part of the solver's reproducibility)
    for (int l = 0; l < n; ++l) s += x[l] * y[l];
    return s;
}

// Cholesky factor of the r x r matrix in R, in place: upper triangular with its strict lower part zero.  false: the factorisation broke down.
inline bool cholesky_upper(std::vector<double> &R, int r)
{
    int info = 0;
    rails_dpotrf('U', r, R.data(), r, &info);
    for (int b = 0; b < r && info == 0; ++b)
        for (int a = b + 1; a < r; ++a) R[a + (size_t)b * r] = 0.0;
    return info == 0;
}

// Cholesky of the Gram matrix G (ldg) restricted to the r rows and columns idx (nullptr: the first r) and scaled to a unit diagonal:
// d = sqrt(diag G), R'R = D^-1 G D^-1, R upper triangular with its strict lower part zero.  false: the factorisation broke down.
// (What the diagonal of G has to satisfy beforehand, and the diagonal of R afterwards, is the caller's to ask.)
inline bool scaled_cholesky(const double *G, int ldg, const int *idx, int r, std::vector<double> &d, std::vector<double> &R)
{
    auto at = [&](int a) { return idx ? idx[a] : a; };
    d.resize(r);
    R.assign((size_t)r * r, 0.0);
    for (int a = 0; a < r; ++a) d[a] = std::sqrt(G[at(a) + (size_t)at(a) * ldg]);
    for (int b = 0; b < r; ++b)
        for (int a = 0; a < r; ++a) R[a + (size_t)b * r] = G[at(a) + (size_t)at(b) * ldg] / (d[a] * d[b]);
    return cholesky_upper(R, r);
}

// Rinv = R^-1 for an upper triangular r x r matrix
inline void upper_inverse(std::vector<double> const &R, int r, std::vector<double> &Rinv)
{
    Rinv.assign((size_t)r * r, 0.0);
    for (int j = 0; j < r; ++j) {
        Rinv[j + (size_t)j * r] = 1.0 / R[j + (size_t)j * r];
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int l = i + 1; l <= j; ++l) s += R[i + (size_t)l * r] * Rinv[l + (size_t)j * r];
            Rinv[i + (size_t)j * r] = -s / R[i + (size_t)i * r];
        }
    }
}

// C = A B for upper triangular r x r matrices (C upper, strict lower part zero).  Scalings are the caller's: a factor that belongs
// inside the sums is applied to the operand beforehand, one that belongs to a whole column to the result afterwards.
inline void upper_product(std::vector<double> const &A, std::vector<double> const &B, int r, std::vector<double> &C)
{
    C.assign((size_t)r * r, 0.0);
    for (int b = 0; b < r; ++b)
        for (int a = 0; a <= b; ++a) {
            double s = 0.0;
            for (int l = a; l <= b; ++l) s += A[a + (size_t)l * r] * B[l + (size_t)b * r];
            C[a + (size_t)b * r] = s;
        }
}

// "Twice is enough" (Kahan / Parlett; the DGKS rule): one projection leaves a component (eps + delta) * ||x|| / ||x'|| along P,
// delta = ||P'P - I||.  Where at least half of a column's squared norm survives that factor is <= sqrt(2) and a second projection has
// nothing to repair.  A looser rule is unstable over long runs: the defect of each new basis column is the old delta times
// ||x|| / ||x'||, and chains of small survivals compound it (measured with 1 %: V'V - I of 1e-14, 2e-12, 6e-7, 0.9 after 50, 100, 200,
// 400 trips of a stagnating solve).
// G0 (w x w, ld w): the block's Gram matrix before the projection; c2[j]: squared length of what the projection found along P.  Returns
// the smallest fraction of a column's squared norm that survives; w2: the second round runs on the columns [0, w2), up to the last one
// that needs it (a zero column or a NaN needs it).
inline double dgks_rule(const double *G0, int w, const double *c2, double threshold, int &w2)
{
    double worst = 1.0;
    w2 = 0;
    for (int j = 0; j < w; ++j) {
        const double g = G0[j + (size_t)j * w];
        const double surv = g > 0.0 ? 1.0 - c2[j] / g : 0.0;
        worst = std::min(worst, surv);
        if (!(surv > threshold)) w2 = j + 1;
    }
    return worst;
}

// The prediction of the overlapped form.  CG (ld dim + w) is what the first round measured: C1 = P'X in its first dim rows, X'X in the
// last w.  The Gram matrix of the projected block follows by Pythagoras, its scaled Cholesky factor gives the block's coordinates along
// its own new basis columns: X - P C1 = Q Rfp, Rfp = R D (w x w, upper).  false: the start conditions are not met.
inline bool predict_block(const double *CG, int dim, int w, std::vector<double> &Rfp)
{
    const int dw = dim + w;
    std::vector<double> Gp((size_t)w * w), d, R;
    for (int j = 0; j < w; ++j)
        for (int i = 0; i <= j; ++i) Gp[i + (size_t)j * w] = Gp[j + (size_t)i * w] = CG[(dim + i) + (size_t)j * dw] - dot(CG + (size_t)i * dw, CG + (size_t)j * dw, dim);
    for (int j = 0; j < w; ++j)
        if (!(Gp[j + (size_t)j * w] > delicate_fraction * CG[(dim + j) + (size_t)j * dw]) || !(Gp[j + (size_t)j * w] > 0.0)) return false;
    if (!scaled_cholesky(Gp.data(), w, nullptr, w, d, R)) return false;
    for (int a = 0; a < w; ++a)
        if (!(R[a + (size_t)a * w] > reproject_diag)) return false; // an ill-conditioned block takes the careful way (re-projection)
    Rfp.assign((size_t)w * w, 0.0);
    for (int b = 0; b < w; ++b)
        for (int a = 0; a <= b; ++a) Rfp[a + (size_t)b * w] = R[a + (size_t)b * w] * d[b];
    return true;
}

// The read-back of the overlapped form.  With X = P (C1 + C2) + Q Rft the truth and (C1, Rfp) what was booked, a vector with booked
// coordinates (a_old, a_new) is P (a_old + C2 Rfp^-1 a_new) + Q (Rft Rfp^-1 a_new): the maps Tn = Rft Rfp^-1 (w x w, upper) and
// To = [C2 0] Rfp^-1 (d0 x w; C2 is d0 x w2, the second round's coefficients).
// off: the largest entry of Tn - I, how far the prediction was off.
struct RebaseMaps { int d0 = 0, w = 0, w2 = 0; double off = 0.0; std::vector<double> Tn, To; };

// G, G2 (w x w): the Gram matrices the device factored in its two CholQR passes (the factors it applied are repeated here on the host's
// copies); g0diag: squared lengths of the block's columns before any projection.  Returns nullptr, or why the block is rejected.
inline const char *rebase_maps(const double *C2, int d0, int w2, const double *G, const double *G2, int w, std::vector<double> const &Rfp,
                               std::vector<double> const &g0diag, RebaseMaps &maps)
{
    const char *const not_full_rank = "the overlapped block orthogonalisation met a block that is not of full rank";
    for (const double *Gm : {G, G2})
        for (int j = 0; j < w; ++j)
            if (!(Gm[j + (size_t)j * w] > 0.0) || !std::isfinite(Gm[j + (size_t)j * w])) return not_full_rank;
    std::vector<double> R1, d1, R2, d2;
    if (!scaled_cholesky(G, w, nullptr, w, d1, R1) || !scaled_cholesky(G2, w, nullptr, w, d2, R2)) return not_full_rank;
    for (int j = 0; j < w; ++j)
        if (!(G[j + (size_t)j * w] > readback_min_fraction * g0diag[j]) || !(R1[j + (size_t)j * w] > readback_min_diag))
            return "the overlapped block orthogonalisation met a block it should have treated with care";
    // Rft = (R2 D2) (R1 D1), upper triangular
    std::vector<double> Rft, Rpi;
    for (int l = 0; l < w; ++l)
        for (int a = 0; a <= l; ++a) R2[a + (size_t)l * w] = R2[a + (size_t)l * w] * d2[l];
    upper_product(R2, R1, w, Rft);
    for (int b = 0; b < w; ++b)
        for (int a = 0; a <= b; ++a) Rft[a + (size_t)b * w] = Rft[a + (size_t)b * w] * d1[b];
    upper_inverse(Rfp, w, Rpi);
    upper_product(Rft, Rpi, w, maps.Tn);
    maps.d0 = d0, maps.w = w, maps.w2 = w2, maps.off = 0.0;
    for (int b = 0; b < w; ++b)
        for (int a = 0; a <= b; ++a) maps.off = std::max(maps.off, std::fabs(maps.Tn[a + (size_t)b * w] - (a == b ? 1.0 : 0.0)));
    if (!(maps.off < readback_max_off)) return "the overlapped block orthogonalisation did not confirm its prediction";
    maps.To.assign((size_t)d0 * w, 0.0);
    if (w2 > 0) rails_dgemm('N', 'N', d0, w, w2, 1.0, C2, d0, Rpi.data(), w, 0.0, maps.To.data(), d0);
    return nullptr;
}

// one coefficient column (at least d0 + w rows) from the predicted new basis columns to the real ones
inline void rebase_column(RebaseMaps const &maps, double *cj)
{
    const int d0 = maps.d0, w = maps.w;
    double *an = cj + d0;
    for (int a = 0; a < w && maps.w2 > 0; ++a) {
        const double x = an[a], *t = maps.To.data() + (size_t)a * d0;
        for (int i = 0; x != 0.0 && i < d0; ++i) cj[i] += t[i] * x;
    }
    for (int a = 0; a < w; ++a) { // (Tn is upper triangular: entry a of the result needs the old entries from a on only, so in place)
        double sum = 0.0;
        for (int l = a; l < w; ++l) sum += maps.Tn[a + (size_t)l * w] * an[l];
        an[a] = sum;
    }
}

} // namespace block_orth
} // namespace rails

#endif
