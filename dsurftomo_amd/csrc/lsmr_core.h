// The scalar part of LSMR (reference lsmrModule.f90:380-651): plane rotations, norm estimates, stopping tests and the
// local-reorthogonalisation queue state of ONE solve, in fp32 exactly as written in the reference.  dsa_lsmr (lsmr.hip)
// keeps one of these; dsa_lsmr_batch (lsmr_batch.hip) keeps one per realisation.  The vector operations stay with the callers,
// which run them in the reference's order around these steps:
//
//   start(alpha, beta)                            after u = b, beta = |u|, u /= beta, v = A'u, alpha = |v|, v /= alpha
//   loop:  itn += 1; u = A v - alpha u; beta = |u|
//          beta > 0:  u /= beta; [enqueue v at enqueue_slot()]; v = A'u - beta v; [ortho over ortho_count() slots];
//                     alpha = |v|; alpha > 0: v /= alpha
//          rotate(); update with c1, c2, c3 (:545-547); normx = |x|; converged(normx)?
//   finish()
#pragma once

#include <cmath>

namespace dsa {

// lsmrModule.f90:686-711
inline float d2norm(float a, float b)
{
    const float scale = fabsf(a) + fabsf(b);
    if (scale == 0.0f) return 0.0f;
    const float p = a / scale, q = b / scale;
    return scale * sqrtf(p * p + q * q);
}

struct LsmrScalars {
    float damp, atol, btol, ctol = 0.0f;
    int itnlim, localVecs;
    bool damped;
    float alpha = 0.0f, beta = 0.0f;
    int itn = 0, istop = 0;
    float normA = 0.0f, condA = 0.0f, normr = 0.0f, normAr = 0.0f, normx = 0.0f;
    bool localOrtho = false, localVQueueFull = false;
    int localPointer = 0;
    float zetabar = 0.0f, alphabar = 0.0f, rho = 1.0f, rhobar = 1.0f, cbar = 1.0f, sbar = 0.0f;
    float betadd = 0.0f, betad = 0.0f, rhodold = 1.0f, tautildeold = 0.0f, thetatilde = 0.0f, zeta = 0.0f, d = 0.0f;
    float normA2 = 0.0f, maxrbar = 0.0f, minrbar = 1e+30f, normb = 0.0f;
    float c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;       // the update of the current iteration, :545-547

    LsmrScalars(float damp_, float atol_, float btol_, float conlim, int itnlim_, int localVecs_)
        : damp(damp_), atol(atol_), btol(btol_), itnlim(itnlim_), localVecs(localVecs_), damped(damp_ > 0.0f)
    {
        if (conlim > 0.0f) ctol = 1.0f / conlim;
    }

    // :397-478 with the first alpha and beta; false when the reference skips the iteration (normAr == 0: x = 0, itn = 0).
    // When it returns true and localOrtho is set, v goes to queue slot 0 (:408-413).
    bool start(float alpha_, float beta_)
    {
        alpha = alpha_; beta = beta_;
        itn = 0; istop = 0; normA = 0.0f; condA = 0.0f; normx = 0.0f;
        normr = beta;
        normAr = alpha * beta;
        if (normAr == 0.0f) return false;
        if (localVecs > 0) { localPointer = 1; localOrtho = true; }
        zetabar = alpha * beta; alphabar = alpha; rho = 1.0f; rhobar = 1.0f; cbar = 1.0f; sbar = 0.0f;
        betadd = beta; betad = 0.0f; rhodold = 1.0f; tautildeold = 0.0f; thetatilde = 0.0f; zeta = 0.0f; d = 0.0f;
        normA2 = alpha * alpha; maxrbar = 0.0f; minrbar = 1e+30f;
        normb = beta;
        return true;
    }

    // localVEnqueue, :715-727 (only when localOrtho and beta > 0): the slot the current v goes to
    int enqueue_slot()
    {
        if (localPointer < localVecs) localPointer += 1;
        else { localPointer = 1; localVQueueFull = true; }
        return localPointer - 1;
    }
    // localVOrtho, :731-748: how many queued v's the new v is orthogonalised against
    int ortho_count() const { return localVQueueFull ? localVecs : localPointer; }

    // plane rotations and estimates with this iteration's alpha and beta, :516-600 in the reference's order (all but normx)
    void rotate()
    {
        const float alphahat = d2norm(alphabar, damp);
        const float chat = alphabar / alphahat, shat = damp / alphahat;
        const float rhoold = rho;
        rho = d2norm(alphahat, beta);
        const float c = alphahat / rho, s = beta / rho;
        const float thetanew = s * alpha;
        alphabar = c * alpha;
        const float rhobarold = rhobar, zetaold = zeta;
        const float thetabar = sbar * rho, rhotemp = cbar * rho;
        rhobar = d2norm(cbar * rho, thetanew);
        cbar = cbar * rho / rhobar;
        sbar = thetanew / rhobar;
        zeta = cbar * zetabar;
        zetabar = -sbar * zetabar;
        c1 = thetabar * rho / (rhoold * rhobarold);
        c2 = zeta / (rho * rhobar);
        c3 = thetanew / rho;
        const float betaacute = chat * betadd, betacheck = -shat * betadd;
        const float betahat = c * betaacute;
        betadd = -s * betaacute;
        const float thetatildeold = thetatilde;
        const float rhotildeold = d2norm(rhodold, thetabar);
        const float ctildeold = rhodold / rhotildeold, stildeold = thetabar / rhotildeold;
        thetatilde = stildeold * rhobar;
        rhodold = ctildeold * rhobar;
        betad = -stildeold * betad + ctildeold * betahat;
        tautildeold = (zetaold - thetatildeold * tautildeold) / rhotildeold;
        const float taud = (zeta - thetatilde * tautildeold) / rhodold;
        d = d + betacheck * betacheck;
        {
            const float e1 = betad - taud;
            normr = sqrtf(d + e1 * e1 + betadd * betadd);
        }
        normA2 = normA2 + beta * beta;
        normA = sqrtf(normA2);
        normA2 = normA2 + alpha * alpha;
        maxrbar = maxrbar > rhobarold ? maxrbar : rhobarold;
        if (itn > 1) minrbar = minrbar < rhobarold ? minrbar : rhobarold;
        condA = (maxrbar > rhotemp ? maxrbar : rhotemp) / (minrbar < rhotemp ? minrbar : rhotemp);
        normAr = fabsf(zetabar);
    }

    // the stopping tests, :601-613, with |x| after this iteration's update: true when the solve stops
    bool converged(float normx_)
    {
        normx = normx_;
        const float test1 = normr / normb;
        const float test2 = normAr / (normA * normr);
        const float test3 = 1.0f / condA;
        const float t1 = test1 / (1.0f + normA * normx / normb);
        const float rtol = btol + atol * normA * normx / normb;
        if (itn >= itnlim) istop = 7;
        if (1.0f + test3 <= 1.0f) istop = 6;
        if (1.0f + test2 <= 1.0f) istop = 5;
        if (1.0f + t1 <= 1.0f) istop = 4;
        if (test3 <= ctol) istop = 3;
        if (test2 <= atol) istop = 2;
        if (test1 <= rtol) istop = 1;
        return istop != 0;
    }

    void finish() { if (damped && istop == 2) istop = 3; }      // :651
};

}  // namespace dsa
