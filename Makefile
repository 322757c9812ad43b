# Top-level build: the HIP library + C++ adapter (product), the CPU oracle and
# the C++ adapter test driver (test infrastructure).
all: hip host oracle oracle_ref cpptest

hip:
	$(MAKE) -C my-lidar-graph-slam_amd/csrc

host: hip
	$(MAKE) -C my-lidar-graph-slam_amd/host

oracle:
	$(MAKE) -C oracle

# the reference's own Eigen/Boost-free sources, compiled in place (test pins)
oracle_ref:
	$(MAKE) -C oracle/ref

cpptest: host oracle
	$(MAKE) -C tests/cpp
	$(MAKE) -C tests/cpp_ge_exact
	$(MAKE) -C tests/cpp_gs
	$(MAKE) -C tests/cpp_hc
	$(MAKE) -C tests/cpp_hc_sq
	$(MAKE) -C tests/cpp_loop_sq
	$(MAKE) -C tests/cpp_pgcg
	$(MAKE) -C tests/cpp_pglm
	$(MAKE) -C tests/cpp_icp
	$(MAKE) -C tests/cpp_icp_ref
	$(MAKE) -C tests/cpp_icp_ref_set
	$(MAKE) -C tests/cpp_icp_window
	$(MAKE) -C tests/cpp_loop_search
	$(MAKE) -C tests/cpp_hv
	$(MAKE) -C tests/cpp_coarse_pair
	$(MAKE) -C tests/cpp_loop
	$(MAKE) -C tests/cpp_pg_cases

clean:
	$(MAKE) -C my-lidar-graph-slam_amd/csrc clean
	$(MAKE) -C my-lidar-graph-slam_amd/host clean
	$(MAKE) -C oracle clean
	$(MAKE) -C oracle/ref clean
	$(MAKE) -C tests/cpp clean
	$(MAKE) -C tests/cpp_ge_exact clean
	$(MAKE) -C tests/cpp_gs clean
	$(MAKE) -C tests/cpp_hc clean
	$(MAKE) -C tests/cpp_hc_sq clean
	$(MAKE) -C tests/cpp_loop_sq clean
	$(MAKE) -C tests/cpp_pgcg clean
	$(MAKE) -C tests/cpp_pglm clean
	$(MAKE) -C tests/cpp_icp clean
	$(MAKE) -C tests/cpp_icp_ref clean
	$(MAKE) -C tests/cpp_icp_ref_set clean
	$(MAKE) -C tests/cpp_icp_window clean
	$(MAKE) -C tests/cpp_loop_search clean
	$(MAKE) -C tests/cpp_hv clean
	$(MAKE) -C tests/cpp_coarse_pair clean
	$(MAKE) -C tests/cpp_loop clean
	$(MAKE) -C tests/cpp_pg_cases clean

.PHONY: all hip host oracle oracle_ref cpptest clean
