"""Coefficients of csrc/nlc_math.h exp_ratio_reduced: e^r ~ (E + r O)/(E - r O) on |r| <= ln2/2 (1 + 1e-6), s = r^2,
E = 1 + c2 s + c4 s^2, O = c1 + c3 s (the shape of the [4/4] Pade approximant).  The relative error of e^r is
2 atanh(r O / E) - r; a Remez exchange on five alternation points in (0, ln2/2] makes it equioscillate, starting from the
Pade coefficients (1/2, 3/28, 1/84, 1/1680).  Prints the Pade error, the minimax error per iteration and the coefficients
(c1, c2, c3, c4) in decimal and as C hex literals.   python tools/exp_ratio_remez.py   (mpmath, CPU, a few seconds)"""
import mpmath as mp
mp.mp.dps = 50
A = mp.log(2)/2 * (1 + mp.mpf('1e-6'))
def err(c, r):
    c1, c2, c3, c4 = c
    s = r*r
    u = r*(c1 + c3*s)/(1 + c2*s + c4*s*s)
    return 2*mp.atanh(u) - r
c = [mp.mpf(1)/2, mp.mpf(3)/28, mp.mpf(1)/84, mp.mpf(1)/1680]
print('pade max', max(abs(err(c, A*i/200)) for i in range(201)))
xs = [A*(1 - mp.cos(mp.pi*(i+1)/5))/2 for i in range(5)]
xs[-1] = A
for it in range(12):
    def eqs(c1, c2, c3, c4, E):
        return [err([c1,c2,c3,c4], x) - (-1)**i*E for i, x in enumerate(xs)]
    sol = mp.findroot(eqs, c + [mp.mpf(0)])
    c = list(sol[:4]); E = sol[4]
    # locate extrema
    N = 2000
    g = [A*i/N for i in range(N+1)]
    v = [err(c, x) for x in g]
    ext = []
    for i in range(1, N):
        if (v[i]-v[i-1])*(v[i+1]-v[i]) < 0:
            ext.append(mp.findroot(lambda x: mp.diff(lambda t: err(c, t), x), g[i]))
    ext.append(A)
    if len(ext) == 5: xs = ext
    print(it, mp.nstr(E, 5), len(ext), mp.nstr(max(abs(x) for x in v), 5))
print([mp.nstr(x, 20) for x in c])
for x in c: print(float(x).hex())
