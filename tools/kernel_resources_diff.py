"""Kernel resources and instruction text of every kernel in two builds of the library, side by side (no GPU needed):

    python tools/kernel_resources_diff.py <parent>/g-meta_amd/csrc/build <this>/g-meta_amd/csrc/build > profiles/<name>.txt

Each build directory holds the objects `python g-meta_amd/build.py` leaves.  Per object the gfx950 code object is unbundled and, per kernel, read as in
tests/test_kernel_resources.py: allocated VGPRs and the granulated SGPR field (compute_pgm_rsrc1 of <kernel>.kd), static LDS and scratch bytes (the first two
words of <kernel>.kd), the size of the kernel's symbol, its instruction count and a digest of its instruction text (llvm-objdump -d without addresses and
encodings; the alignment padding behind the last instruction is left out).  Kernels are matched by demangled name without the argument list: `same` =
every figure and the digest equal, `DIFFERS`, `new`, `removed` (a kernel that became a template shows as removed + new under its new name: compare the two lines)."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM_BIN', '/opt/rocm/lib/llvm/bin')
def dev_elf(obj,tmp):
    fb,dev=os.path.join(tmp,'fb.bin'),os.path.join(tmp,os.path.basename(obj)+'.dev')
    if subprocess.run([LLVM+'/llvm-objcopy','--dump-section','.hip_fatbin='+fb,obj],capture_output=True).returncode: return None
    subprocess.run([LLVM+'/clang-offload-bundler','--unbundle','--type=o','--input='+fb,'--targets=hipv4-amdgcn-amd-amdhsa--gfx950','--output='+dev],check=True,cwd=tmp)
    return dev
def fin(buf):
    while buf and (buf[-1].startswith('s_nop') or buf[-1]=='...'): buf=buf[:-1]
    return (len(buf),hashlib.md5('\n'.join(buf).encode()).hexdigest()[:8])
def info(dev):
    sec=subprocess.run([LLVM+'/llvm-readelf','-S','-W',dev],check=True,capture_output=True,text=True).stdout
    m=re.search(r'\]\s+\.rodata\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)',sec)
    addr,off,size=(int(x,16) for x in m.groups())
    data=open(dev,'rb').read()
    sym=subprocess.run([LLVM+'/llvm-readelf','-s','-W',dev],check=True,capture_output=True,text=True).stdout
    kd={};fn={}
    for line in sym.splitlines():
        f=line.split()
        if len(f)>=8:
            if f[-1].endswith('.kd'):
                a=int(f[1],16)
                lds,scr=struct.unpack_from('<II',data,off+(a-addr))
                r1=struct.unpack_from('<I',data,off+(a-addr)+48)[0]
                kd[f[-1][:-3]]=(((r1&0x3f)+1)*8,(r1>>6)&0xf,lds,scr)
            elif f[3]=='FUNC':
                fn[f[-1]]=int(f[2])
    dis=subprocess.run([LLVM+'/llvm-objdump','-d','--no-show-raw-insn','--no-leading-addr',dev],check=True,capture_output=True,text=True).stdout
    h={};cur=None;buf=[]
    for line in dis.splitlines():
        m=re.match(r'^[0-9a-f]* ?<(.+)>:$',line.strip())
        if m:
            if cur: h[cur]=fin(buf)
            cur=m.group(1);buf=[]
        elif line.strip() and cur is not None:
            buf.append(re.sub(r'//.*','',line).strip())
    if cur: h[cur]=fin(buf)
    return {k:kd[k]+(fn.get(k,0),)+h.get(k,('?',0)) for k in kd}
def all_info(build):
    out={}
    with tempfile.TemporaryDirectory() as tmp:
        for o in sorted(os.listdir(build)):
            if o.endswith('.o'):
                d=dev_elf(os.path.join(build,o),tmp)
                if d is None: continue
                for k,v in info(d).items(): out[(o,k)]=v
    return out
a=all_info(sys.argv[1]); b=all_info(sys.argv[2])
names=sorted(set(k[1] for k in list(a)+list(b)))
dm=dict(zip(names,subprocess.run(['c++filt']+names,check=True,capture_output=True,text=True).stdout.split('\n')))
def rekey(d): return {(k[0],re.sub(r'\(.*','',dm[k[1]]).replace('void ','')):v for k,v in d.items()}
a=rekey(a); b=rekey(b)
same=diff=0
print('columns: VGPRs, granulated SGPR field, static LDS bytes, scratch bytes, code bytes, instructions, md5 of the instruction text (first 8 hex digits)')
for k in sorted(set(a)|set(b)):
    n=k[1]
    if k in a and k in b:
        if a[k]==b[k]: same+=1; print('same     %-16s %-58s %s'%(k[0],n,' '.join(map(str,a[k]))))
        else: diff+=1; print('DIFFERS  %-16s %-58s parent %s | this %s'%(k[0],n,' '.join(map(str,a[k])),' '.join(map(str,b[k]))))
    elif k in b: print('new      %-16s %-58s %s'%(k[0],n,' '.join(map(str,b[k]))))
    else: print('removed  %-16s %-58s %s'%(k[0],n,' '.join(map(str,a[k]))))
print('pre-existing kernels identical: %d, differing: %d'%(same,diff))
