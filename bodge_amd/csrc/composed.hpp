// composed.hpp - host arithmetic of the composed three-step sweep (sweep.hpp K7b, COMP): from the dot products a
// run of composed sweeps leaves behind to the d_n = <t_n|t_n>, e_n = <t_{n+1}|t_n> every caller expects.
// Host only, no device code and no HIP call: exported as bdg_host_composed_dots, so that a test can drive it without a GPU.
//
// A composed sweep starts at c = 3k from u = t_c and makes w_j = T_j(H~) u = (t_{c+j} + t_{c-j}) / 2, j = 1..3 (t_{-m} = t_m in
// the sense of the moments: at c = 0 the w_j are t_j).  Row n = c + j of the run's dot table then holds
//     a = <w_j|w_j>,  b = <w_{j+1}|w_j>            instead of d_n, e_n.
// With mu_m = <t_0|t_m> (mu_{2n} = 2 d_n - d_0, mu_{2n+1} = 2 e_n - e_0) and <t_p|t_q> = (mu_{p+q} + mu_{|p-q|}) / 2,
//     8 <w_i|w_j> = sum over the four sign pairs of  mu_{A+B} + mu_{|A-B|},   A = |c +- i|, B = |c +- j|,
// and of the eight moments on the right exactly the highest, mu_{2c+i+j} = mu_{2n} (a) or mu_{2n+1} (b), is new: every
// other one belongs to an earlier row.  So the rows are turned back in order, each new moment = 8 x the measured sum
// minus older moments (divided by how often it occurs: once, at c = 0 up to four times).  Errors add, nothing amplifies them.
// d_{3k} = <u|u> is the kernel's own number and is handed through untouched.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <vector>

namespace bdg_host {

// One vector: raw[n * raw_stride + {0, 1}] = (a, b) of row n < n_steps;  d[n * out_stride], e[n * out_stride] receive d_n, e_n.
// Any run length: the last sweep may have 1 or 2 rows only.
inline void composed_dots_vector(int n_steps, const double* raw, size_t raw_stride, double* d, double* e, size_t out_stride) {
    std::vector<double> mu((size_t)2 * n_steps);
    for (int n = 0; n < n_steps; ++n) {
        const int j = n % 3, c = n - j;
        for (int h = 0; h < 2; ++h) {  // h = 0: <w_j|w_j>, h = 1: <w_{j+1}|w_j>
            const int i = j + h, target = 2 * c + i + j;  // (= 2n + h)
            const double measured = raw[(size_t)n * raw_stride + h];
            if (i == 0) {  // <u|u> = d_c itself
                mu[(size_t)target] = c == 0 ? measured : 2.0 * measured - mu[0];
                continue;
            }
            double older = 0.0;
            int count = 0;
            for (int si = 1; si >= -1; si -= 2)
                for (int sj = 1; sj >= -1; sj -= 2) {
                    const int a = std::abs(c + si * i), b = std::abs(c + sj * j);
                    for (int index : {a + b, std::abs(a - b)}) {
                        if (index == target) ++count;
                        else older += mu[(size_t)index];
                    }
                }
            mu[(size_t)target] = (8.0 * measured - older) / count;
        }
    }
    for (int n = 0; n < n_steps; ++n) {
        d[(size_t)n * out_stride] = n % 3 == 0 ? raw[(size_t)n * raw_stride] : 0.5 * (mu[(size_t)2 * n] + mu[0]);
        e[(size_t)n * out_stride] = 0.5 * (mu[(size_t)2 * n + 1] + mu[1]);
    }
}

}  // namespace bdg_host
