"""The known answer of the forward-walking test (tests/test_gpu_dmc_observables.py): <V_en> and <V_ee> of the lowest antisymmetric eigenstate
of the 1-D soft-Coulomb helium Hamiltonian in the box [-10, 10]^2 -- the Hamiltonian and the finite-difference grid of scratch/he1d_exact.py,
at n = 300 and n = 400 points per axis.  The eigenvector is normalised on the grid, so an expectation value is sum |P|^2 V."""
import numpy as np, scipy.sparse as sp, scipy.sparse.linalg as sla
L = 10.0
for n in (300, 400):
    x = np.linspace(-L, L, n + 2)[1:-1]          # Dirichlet walls
    h = x[1] - x[0]
    T1 = sp.diags([-0.5 / h**2, 1.0 / h**2, -0.5 / h**2], [-1, 0, 1], shape=(n, n))   # -1/2 d^2/dx^2
    I = sp.identity(n)
    X1, X2 = np.meshgrid(x, x, indexing="ij")
    V_en = -2 / np.sqrt(1 + X1**2) - 2 / np.sqrt(1 + X2**2)
    V_ee = 1 / np.sqrt(1 + (X1 - X2)**2)
    H = sp.kron(T1, I) + sp.kron(I, T1) + sp.diags((V_en + V_ee).ravel())
    w, v = sla.eigsh(H.tocsc(), k=4, which="SA")
    for e, vec in zip(w, v.T):
        P = vec.reshape(n, n)
        if np.linalg.norm(P - P.T) / np.linalg.norm(P) > 1:    # ~0: symmetric (singlet), ~2: antisymmetric (triplet)
            p2 = P**2 / (P**2).sum()
            print(f"L={L} n={n} h={h:.4f}: E {e:.5f}  <V_en> {(p2 * V_en).sum():.5f}  <V_ee> {(p2 * V_ee).sum():.5f}  "
                  f"<T> {e - (p2 * (V_en + V_ee)).sum():.5f}")
            break
