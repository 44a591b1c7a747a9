# tests/cpp/test_upload_host: the host-only parts of loading voxels back into the dense map
# (form_amd/csrc/upload_host.hpp, no HIP headers), plain g++ -Werror like its neighbours, with
# the address and undefined-behaviour sanitizers (runtimes linked statically: the program needs
# nothing preloaded).
# Built by __graft_entry__.build():  make -C tests/cpp -f upload_host.mk
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
	-static-libasan -static-libubsan
all: test_upload_host
test_upload_host: test_upload_host.cpp $(ROOT)/form_amd/csrc/upload_host.hpp $(ROOT)/include/fmx/fmx.h
	$(CXX) $(CXXFLAGS) -I$(ROOT)/form_amd/csrc -I$(ROOT)/include -o $@ test_upload_host.cpp
clean:
	rm -f test_upload_host
.PHONY: all clean
