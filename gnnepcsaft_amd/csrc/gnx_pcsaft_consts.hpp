// Published constants of the pure-component PC-SAFT used by gnx_pcsaft.hip (data, typed from the papers).
//
// Dispersion: Gross, J.; Sadowski, G. "Perturbed-Chain SAFT: An Equation of State Based on a Perturbation Theory for
// Chain Molecules", Ind. Eng. Chem. Res. 40 (2001) 1244-1260, Table 1 (universal model constants a_0i .. b_2i,
// i = 0..6).  a_i(m) = a_0i + (m-1)/m a_1i + (m-1)/m (m-2)/m a_2i, likewise b_i(m).
//
// Dipole: Gross, J.; Vrabec, J. "An Equation-of-State Contribution for Polar Components: Dipolar Molecules",
// AIChE J. 52 (2006) 1194-1204, Table 1 (a_0n .. c_2n, n = 0..4; b_n3 = b_n4 = c_n4 = 0).
//
// tests/pcsaft_ref.py types the same tables a second time and tests/test_pcsaft_cpu.py compares the two digit for digit.
#pragma once

namespace gnx_pcsaft {

// SI 2019 exact values
constexpr double kAvogadro = 6.02214076e23;  // 1/mol
constexpr double kBoltzmann = 1.380649e-23;  // J/K
// mu*^2 = mu^2 / (m eps/k sigma^3) * kDipoleFactor with mu in debye, eps/k in K, sigma in angstrom (the factor of the
// note under Gross & Vrabec's Table 2)
constexpr double kDipoleFactor = 7242.702976750923;
// close packing of spheres, pi / (3 sqrt 2): upper end of every packing-fraction bracket
constexpr double kEtaMax = 0.7405;

// Gross & Sadowski 2001, Table 1
constexpr double kDispA[3][7] = {
    {0.9105631445, 0.6361281449, 2.6861347891, -26.547362491, 97.759208784, -159.59154087, 91.297774084},
    {-0.3084016918, 0.1860531159, -2.5030047259, 21.419793629, -65.255885330, 83.318680481, -33.746922930},
    {-0.0906148351, 0.4527842806, 0.5962700728, -1.7241829131, -4.1302112531, 13.776631870, -8.6728470368},
};
constexpr double kDispB[3][7] = {
    {0.7240946941, 2.2382791861, -4.0025849485, -21.003576815, 26.855641363, 206.55133841, -355.60235612},
    {-0.5755498075, 0.6995095521, 3.8925673390, -17.215471648, 192.67226447, -161.82646165, -165.20769346},
    {0.0976883116, -0.2557574982, -9.1558561530, 20.642075974, -38.804430052, 93.626774077, -29.666905585},
};

// Gross & Vrabec 2006, Table 1
constexpr double kDipA[3][5] = {
    {0.3043504, -0.1358588, 1.4493329, 0.3556977, -2.0653308},
    {0.9534641, -1.8396383, 2.0131180, -7.3724958, 8.2374135},
    {-1.1610080, 4.5258607, 0.9751222, -12.281038, 5.9397575},
};
constexpr double kDipB[3][5] = {
    {0.2187939, -1.1896431, 1.1626889, 0.0, 0.0},
    {-0.5873164, 1.2489132, -0.5085280, 0.0, 0.0},
    {3.4869576, -14.915974, 15.372022, 0.0, 0.0},
};
constexpr double kDipC[3][5] = {
    {-0.0646774, 0.1975882, -0.8087562, 0.6902849, 0.0},
    {-0.9520876, 2.9924258, -2.3802636, -0.2701261, 0.0},
    {-0.6260979, 1.2924686, 1.6542783, -3.4396744, 0.0},
};

}  // namespace gnx_pcsaft
