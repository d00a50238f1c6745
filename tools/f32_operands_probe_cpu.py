#!/usr/bin/env python3
"""CPU study behind Hierarchy.set_operand_precision: the fused zero-guess V(1,1) with the operands Ahat = A diag(wd) and A P rounded to
float32 on the first F levels (F = 0, 1, 2, all), arithmetic FP64 — cycle output against the FP64 cycle and BiCGSTAB iterations to 1e-10
(hierarchy from the oracle's aggregation "10 2 8", omega = 0.6).
usage: f32_operands_probe_cpu.py poisson|csky3d N"""
import os, sys, numpy as np, scipy.sparse as sps, scipy.sparse.linalg as spla
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle_py as orc
from multigridsolver_amd.synthetic import csky3d, CSKY_ROWSUM_MARGIN
kind=sys.argv[1]; N=int(sys.argv[2]); n=N**3
if kind=='poisson':
    I=sps.identity(N); T=sps.diags([-1,2,-1],[-1,0,1],shape=(N,N))
    A=(sps.kron(sps.kron(T,I),I)+sps.kron(sps.kron(I,T),I)+sps.kron(sps.kron(I,I),T)).tocsr()
else:
    rp,ci,v=csky3d(N,rowsum_floor=CSKY_ROWSUM_MARGIN); A=sps.csr_matrix((v,ci,rp),shape=(n,n))
As=[A];Ps=[]
while As[-1].shape[0]>2500 and len(As)<10:
    M=As[-1].tocsr(); M.sort_indices()
    Ao=orc.Csr.from_arrays(M.shape[0],M.shape[0],M.indptr.astype(np.int32),M.indices.astype(np.int32),M.data)
    P=Ao.agmg(10.0,2,8.0,strict=False).to_scipy().tocsr()
    Ps.append(P); As.append((P.T@M@P).tocsr())
print(kind,"levels",[a.shape[0] for a in As])
lu=spla.splu(As[-1].tocsc()); w=0.6
wd=[w/a.diagonal() for a in As]
def rnd(m,f):
    m=m.tocsr().copy()
    if f: m.data=m.data.astype(np.float32).astype(np.float64)
    return m
def build(F):
    Ah=[rnd(As[l]@sps.diags(wd[l]),l<F) for l in range(len(Ps))]
    AP=[rnd(As[l]@Ps[l],l<F) for l in range(len(Ps))]
    return Ah,AP
def cyc(Ah,AP,l,b):
    if l==len(As)-1: return lu.solve(b)
    r=b-Ah[l]@b; t=b+r
    ec=cyc(Ah,AP,l+1,Ps[l].T@r)
    return Ps[l]@ec+wd[l]*(t-AP[l]@ec)
rng=np.random.default_rng(0); b=rng.random(n)
ref=None
for F in (0,1,2,99):
    Ah,AP=build(F)
    z=cyc(Ah,AP,0,b)
    if ref is None: ref=z
    its=[0]
    def cb(x): its[0]+=1
    M=spla.LinearOperator((n,n),matvec=lambda r: cyc(Ah,AP,0,r))
    x,info=spla.bicgstab(A,b,M=M,rtol=1e-10,maxiter=500,callback=cb)
    print("f32 levels",F,"cycle rel diff vs f64 %.2e"%(np.linalg.norm(z-ref)/np.linalg.norm(ref)),"bicgstab its",its[0],"info",info,"true res %.2e"%(np.linalg.norm(b-A@x)/np.linalg.norm(b)),flush=True)
